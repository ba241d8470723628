"""The solver kernels at every length and step-count dispatch edge.

The vector kernels under the solvers (reductions, the three MGS forms, the Krylov GEMV and
reconstruction, the Golub-Kahan updates) choose their path from the Krylov dimension, the iteration
budget and a handful of context options.  The tomography problems of the other GPU tests fix
n = N^2 (N even), short runs and default options; this file sweeps the lengths and budgets
themselves, on an operator of any m x n:

  1. a CPU test that ties LENGTHS / MAXITS to the constants of csrc/ (read by regular expression);
  2. a length sweep through 8 Arnoldi steps, both sides, default and mgs_single = 0;
  3. one problem above every grid cap (n = m = 1,049,601), the sweep's three tile widths;
  4. the whole solvers at odd lengths just past the one-workgroup and one-launch limits;
  5. long runs across step MGS1_MAXC = 120 (the one-reduction -> pass-form hand-over);
  6. the pipeline and hand-over options at a small size;
  7. HGM_DEVICE_PTRS on one context, and the refusal of a pointer that is not 16-byte aligned.

The operator is a 1-D Gaussian blur: row i centred at round(i (n-1)/(m-1)), weights
exp(-(o/sigma)^2 / 2) over |o| <= half cut at the borders, rows normalised to sum 1, B = A'.  For
n > m the width is scaled by r = (n-1)/(m-1) (sigma r, half r), i.e. it is measured on the coarser
of the two grids: with the unscaled width the rows of a wide operator do not overlap, A*A' is
diagonal with two distinct values and the oracle's Arnoldi breaks down at its second step (measured:
H(3,2) = 2e-15 at 1537 x 24577 and 1537 x 131073), so no 8-step or 12-step run exists to compare.

The oracle (oracle/restatement.py, fp64 numpy) is the reference throughout.  Its own rounding spread
under test_gpu_parity._Rounded (8 seeds), measured on the CPU for the inputs of sections 4 and 5, is
quoted at each section.
"""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import hgmres
from hgmres import _lib as L
from oracle import restatement as R
from test_gpu_fused import _Rounded32
from test_gpu_parity import GKB_CAP, TOL, H_ok, _gkb_check, _Rounded, hist_ok, rel

gpu = pytest.mark.gpu

FIXED = 1537                        # the dimension that is not swept: small and odd
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 257, 511, 513, 4095, 4096, 4097, 12287, 12289, 16385, 20479, 20481,
           24575, 24576, 24577, 32767, 32768, 32769, 131071, 131073)
CAPPED = 1049601                    # odd, > 2^20: above the MAX_PARTS cap of every reduction grid
SHAPES = ((1537, 24577), (24577, 1537), (32769, 32769))        # section 4
LONG_SHAPES = ((2049, 1537), (4097, 4097))                     # section 5
SMALL = (1537, 4097)                                           # sections 6 and 7
MAXITS = (3, 8, 12, 120, 121, 124)  # Arnoldi steps / iteration budgets the file runs
# lambda of the hybrid solvers.  The blur's B*A has norm ~0.06 at 1537 x 24577; with lambda = 1e-2 the oracle's
# own 12-step H of hybrid_*_gmres_rtp spreads by 1.3e-10 under the rounding model there (the loss of
# orthogonality to the first vector doubles per step), with 1e-4 by 5e-13.
LAM = 1e-4


def blur_problem(m, n, sigma=1.5, half=6, seed=0, noise=1e-2):
    """(A, B = A', b, x_true): the module docstring's blur, x_true = sine + step + offset + 0.3 randn,
    b = A x_true + 1 % noise."""
    r = max(1.0, (n - 1) / max(m - 1, 1))
    sig, hw = sigma * r, int(np.ceil(half * r))
    i = np.arange(m)
    c = np.rint(i * ((n - 1) / (m - 1))).astype(np.int64) if m > 1 else np.zeros(1, np.int64)
    o = np.arange(-hw, hw + 1)
    cols = c[:, None] + o[None, :]
    ok = (cols >= 0) & (cols < n)
    w = np.exp(-0.5 * (o / sig) ** 2)[None, :] * ok
    w /= w.sum(axis=1, keepdims=True)
    A = sp.csr_matrix((w[ok], (np.broadcast_to(i[:, None], cols.shape)[ok], cols[ok])), shape=(m, n))
    A.sort_indices()
    B = A.T.tocsr()
    B.sort_indices()
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)
    xt = np.sin(6 * np.pi * t) + (t > 0.5) + 2.0 + 0.3 * rng.standard_normal(n)
    b = A @ xt
    e = rng.standard_normal(m)
    return A, B, b + noise * np.linalg.norm(b) / np.linalg.norm(e) * e, xt


@functools.lru_cache(maxsize=None)
def _problem(m, n):
    return blur_problem(m, n)


@contextlib.contextmanager
def _device_ops(ctx, A, B, dtype=L.HGM_F64):
    Ao = hgmres.SparseOperator.from_scipy(A, ctx, dtype=dtype)
    Bo = hgmres.SparseOperator.from_scipy(B, ctx, dtype=dtype)
    try:
        yield Ao, Bo
    finally:
        Ao.close()
        Bo.close()


# (tag, device solver, oracle, takes lambda)
GM = {"hab": (hgmres.hybrid_ab_gmres_rtp, R.hybrid_ab_gmres_rtp, True),
      "hba": (hgmres.hybrid_ba_gmres_rtp, R.hybrid_ba_gmres_rtp, True),
      "abp": (hgmres.ABgmres_hybrid_bounds, R.ABgmres_hybrid_bounds, True),
      "abn": (hgmres.ABgmres_nonhybrid_bounds, R.ABgmres_nonhybrid_bounds, False),
      "bap": (hgmres.BAgmres_hybrid_bounds, R.BAgmres_hybrid_bounds, True),
      "ban": (hgmres.BAgmres_nonhybrid_bounds, R.BAgmres_nonhybrid_bounds, False)}


def _gm_gpu(ctx, tag, Ao, Bo, b, xt, maxit, tol=0.0, **opts):
    """(x, err, res, niters, H) of one device solve under the context options `opts`."""
    fn, _, haslam = GM[tag]
    with ctx.options(**opts):
        o = fn(Ao, Bo, b, xt, tol, maxit, *((LAM,) if haslam else ()), ctx=ctx, return_H=True)
    return o[0], o[1], o[2], o[3], o[-1]


def _gm_ref(tag, A, B, b, xt, maxit, tol=0.0):
    _, fn, haslam = GM[tag]
    o = fn(A, B, b, xt, tol, maxit, *((LAM,) if haslam else ()), return_H=True)
    return o[0], o[1], o[2], o[3], o[-1]


def _gm_dev(out, ref):
    """Deviations (H against max|H|, x in norm, the two histories per entry) of a solve from a reference."""
    assert out[3] == ref[3], (out[3], ref[3])
    with np.errstate(invalid="ignore", divide="ignore"):
        hd = [float(np.max(np.abs(np.asarray(out[i]) - np.asarray(ref[i])) / np.abs(np.asarray(ref[i]))))
              for i in (1, 2)]
    return dict(H=float(np.max(np.abs(out[4] - ref[4])) / np.max(np.abs(ref[4]))), x=float(rel(out[0], ref[0])),
                err=hd[0], res=hd[1])


def _gm_ok(out, ref, tol, what=""):
    assert out[3] == ref[3], (what, out[3], ref[3])
    H_ok(out[4], ref[4], tol)
    assert rel(out[0], ref[0]) < tol, (what, rel(out[0], ref[0]))
    hist_ok(out[1], ref[1], tol)
    hist_ok(out[2], ref[2], tol)


def _bitwise(a, b):
    return a[3] == b[3] and all(np.array_equal(np.asarray(a[i]), np.asarray(b[i])) for i in (0, 1, 2, 4))


# ---------------------------------------------------------------------------------------------
# 1. the lengths and budgets against the constants of csrc/
# ---------------------------------------------------------------------------------------------
def _csrc_constants():
    """SINGLE_MAX, MGS1_BS, MGS1_MAX, MGS1_MAXC, MAX_PARTS, BS and the mgs1_tile thresholds
    [(pairs, P), ...] as csrc/ states them."""
    src = ""
    for f in ("internal.h", "device_common.h", "kernels.hip"):
        with open(os.path.join(ROOT, "hybrid-gmres_amd", "csrc", f)) as fh:
            src += fh.read()
    vals = {}
    for name in ("BS", "MAX_PARTS", "SINGLE_MAX", "MGS1_BS", "MGS1_MAX", "MGS1_MAXC"):
        mt = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert mt, name
        expr = mt.group(1)
        assert re.fullmatch(r"[\w\s*+<()-]+", expr), (name, expr)
        vals[name] = int(eval(expr, {"__builtins__": {}}, dict(vals)))
    body = re.search(r"static int mgs1_tile\([^)]*\)\s*\{(.*?)\n\}", src, re.S)
    assert body, "mgs1_tile"
    tiles = [(vals["BS"] * int(a) * int(b), int(p))
             for a, b, p in re.findall(r"n2 >= \(int64_t\)BS \* (\d+) \* (\d+) \? (\d+)", body.group(1))]
    assert len(tiles) == 2 and "n2 = n >> 1" in body.group(1), body.group(1)
    return vals, tiles


def test_lengths_cover_the_dispatch_edges():
    """Every edge below is the largest length (or budget) of its low side.  The lengths the file runs hold
    a value and an odd value on each side of each, the edge itself and its successor where a kernel hands
    over to another at it, and a length inside every k_mgs_single instantiation.  A constant that moves in
    csrc/ fails this test instead of silently leaving its edge uncovered."""
    v, tiles = _csrc_constants()
    lengths = sorted(set(LENGTHS) | {CAPPED, FIXED} | {d for s in SHAPES + LONG_SHAPES + (SMALL,) for d in s})
    BS, MP = v["BS"], v["MAX_PARTS"]
    assert v["MGS1_MAX"] % (4 * v["MGS1_BS"]) == 0
    singles = [4 * v["MGS1_BS"] * j for j in range(1, v["MGS1_MAX"] // (4 * v["MGS1_BS"]) + 1)]
    edges = {"one block of pair lanes (2 BS)": 2 * BS, "one block of lanes (BS)": BS,
             "SINGLE_MAX": v["SINGLE_MAX"], "MGS1_MAX": v["MGS1_MAX"],
             "parts_for cap": 4 * BS * MP, "gemv_blocks / mgs1 P=1 cap": 2 * BS * MP + 1,
             "mgs1 P=2 cap": 4 * BS * MP + 1}
    for pairs, P in tiles:
        edges[f"mgs1_tile P={P}"] = 2 * pairs - 1
    for j, e in enumerate(singles):
        edges[f"k_mgs_single E={4 * (j + 1)}"] = e
    for name, e in edges.items():
        lo, hi = [x for x in lengths if x <= e], [x for x in lengths if x > e]
        assert lo and hi, (name, e)
        assert any(x % 2 for x in lo) and any(x % 2 for x in hi), (name, e)
    for name in ("SINGLE_MAX", "MGS1_MAX"):                       # the exact hand-over
        assert v[name] in lengths and v[name] + 1 in lengths and v[name] - 1 in lengths, name
    for lo, hi in zip([0] + singles[:-1], singles):               # every instantiation runs
        assert any(lo < x <= hi for x in LENGTHS), (lo, hi)
    # the auto tile width takes each of its values, and the forced widths 1 and 2 run above their grid cap
    auto = lambda n: next((P for pairs, P in tiles if (n >> 1) >= pairs), 1)   # noqa: E731
    assert {auto(x) for x in lengths} == {1, 2, 4} and auto(CAPPED) == 4
    for P in (1, 2):
        assert ((CAPPED >> 1) + BS * P - 1) // (BS * P) > MP, P
    assert (CAPPED + 4 * BS - 1) // (4 * BS) > MP and CAPPED % 2 == 1 and CAPPED > 1 << 20
    # the iteration budgets around MGS1_MAXC
    c = v["MGS1_MAXC"]
    assert c in MAXITS and c + 1 in MAXITS and max(MAXITS) > c + 1
    assert any(k % 2 and k <= c for k in MAXITS) and any(k % 2 and k > c for k in MAXITS)


# ---------------------------------------------------------------------------------------------
# 2. length sweep through Arnoldi
# ---------------------------------------------------------------------------------------------
def _kdone(H):
    nz = np.flatnonzero(np.any(H != 0, axis=0))
    return int(nz[-1]) + 1 if nz.size else 0


@gpu
@pytest.mark.parametrize("side", ["ba", "ab"])
@pytest.mark.parametrize("length", LENGTHS)
def test_arnoldi_length_sweep(gpu_ctx, length, side):
    """8 MGS Arnoldi steps (gcv_function.m:3-33) with the Krylov dimension swept -- n for `ba`, m for `ab` --
    and the other dimension 1537, against the oracle: H at 1e-10 of max|H|, beta at 1e-13.  Default options,
    and mgs_single = 0 (the multi-block forms) up to MGS1_MAX.
    Lengths below 14 cannot carry 8 steps: the oracle breaks down (:30), and the device must stop at the same
    step and keep the same zero columns (:33).  There the last subdiagonal entry is rounding noise of size
    eps |B*A| ~ 5e-13 (1537 x 2), next to the reference's absolute threshold 1e-12, so both sides are given
    the threshold 1e-9: three orders above that noise, eight below the genuine entries."""
    k = 8
    m, n = (FIXED, length) if side == "ba" else (length, FIXED)
    A, B, b, _ = blur_problem(m, n)
    bd = 1e-9 if length < 14 else 1e-12
    Hr, br = R.arnoldi(A, B, b, k, side, breakdown_tol=bd)
    kr = _kdone(Hr)
    assert kr == (k if length >= 14 else min(length, k)), (kr, length)
    settings = [{}] + ([dict(mgs_single=0)] if length <= 24576 else [])
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        for opts in settings:
            with gpu_ctx.options(**opts):
                H, beta, kd = hgmres.arnoldi(Ao, Bo, b, k, side, ctx=gpu_ctx, breakdown_tol=bd)
            dH = np.max(np.abs(H - Hr)) / np.max(np.abs(Hr))
            print(f"[arnoldi {side} {length} {opts}] kdone {kd} |dH| {dH:.2e} |dbeta| {abs(beta - br) / br:.2e}")
            assert kd == kr, (opts, kd, kr)
            assert np.all(H[:, kd:] == 0) and np.array_equal(H[:, kd:] == 0, Hr[:, kd:] == 0), opts
            H_ok(H, Hr)
            assert abs(beta - br) <= 1e-13 * br, (opts, abs(beta - br) / br)


# ---------------------------------------------------------------------------------------------
# 3. the capped grids, once
# ---------------------------------------------------------------------------------------------
@gpu
def test_capped_grids_once(gpu_ctx):
    """n = m = 1,049,601 (odd, > 2^20): every reduction grid is capped at MAX_PARTS and loops grid-stride,
    and so does the one-reduction sweep with 1 or 2 pairs per lane (auto: 4, 513 tiles).  3 Arnoldi steps,
    BA side, each tile width against the oracle at 1e-10 and against one another at 1e-12 (the partial sums
    are grouped differently, so they are not bitwise equal)."""
    A, B, b, _ = blur_problem(CAPPED, CAPPED, half=2)
    Hr, br = R.arnoldi(A, B, b, 3, "ba")
    outs = {}
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        for ppl in (0, 1, 2):
            with gpu_ctx.options(mgs1_ppl=ppl):
                outs[ppl] = hgmres.arnoldi(Ao, Bo, b, 3, "ba", ctx=gpu_ctx)
    for ppl, (H, beta, kd) in outs.items():
        print(f"[capped ppl {ppl}] |dH| {np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.2e} |dbeta| {abs(beta - br) / br:.2e}")
        assert kd == 3
        H_ok(H, Hr)
        assert abs(beta - br) <= TOL * br
    for p, q in ((0, 1), (0, 2), (1, 2)):
        H_ok(outs[p][0], outs[q][0], 1e-12)
        assert abs(outs[p][1] - outs[q][1]) <= 1e-12 * outs[q][1]


# ---------------------------------------------------------------------------------------------
# 4. whole solvers at odd lengths
#    Oracle spread under _Rounded (8 seeds; BAgmres_nonhybrid_bounds forms B*A explicitly, so a 1-ulp
#    perturbed copy of the operator values instead), 12 iterations, lambda = LAM, measured on the CPU, largest
#    over H, x and both histories:
#                       hab      hba      abp      abn      bap      ban
#      1537 x 24577   5.4e-13  5.4e-13  3.2e-14  3.2e-14  9.5e-13  4.4e-13
#      24577 x 1537   8.3e-13  8.3e-13  1.2e-13  1.3e-14  4.3e-13  2.3e-13
#      32769 x 32769  1.8e-13  1.8e-13  2.6e-14  1.3e-14  1.9e-13  1.0e-13
#    Every family <= 1e-12, which keeps the project's 100x margin under the 1e-10 bar.  Golub-Kahan fp64:
#    x <= 8.3e-15, histories <= 6.8e-14 on the three shapes, so every entry is judged far under the 1e-6 cap.
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("tag", list(GM))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gmres_family_odd_lengths(gpu_ctx, shape, tag):
    """12 iterations, tol = 0: both spaces just past the one-workgroup limit (24577) or the one-launch
    reduction limit (32769), odd.  1e-10 on H, x and both histories."""
    A, B, b, xt = _problem(*shape)
    ref = _gm_ref(tag, A, B, b, xt, 12)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        out = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12)
    print(f"[odd {tag} {shape}] " + " ".join(f"{k}={v:.1e}" for k, v in _gm_dev(out, ref).items()))
    assert out[3] == 12
    _gm_ok(out, ref, TOL, tag)


OPTION_SETTINGS = ([dict(mgs_form=0), dict(mgs_fused=0), dict(pend_norm=0), dict(gram_err=0)]
                   + [dict(mgs1_ppl=p) for p in (1, 2, 4)] + [dict(mgs_ppl=p) for p in range(1, 9)])


@gpu
@pytest.mark.parametrize("tag", list(GM))
def test_gmres_family_options_at_odd_length(gpu_ctx, tag):
    """1537 x 24577 (the n-space basis is multi-block and odd): each sweep option against the oracle at 1e-10
    and its H against the default's at 1e-12; mgs_fused = 0 bitwise equal to the default (same summation
    code).  mgs_ppl over every value hgm_ctx_set_option accepts (1..8)."""
    A, B, b, xt = _problem(*SHAPES[0])
    ref = _gm_ref(tag, A, B, b, xt, 12)
    with pytest.raises(ValueError):
        gpu_ctx.set_option("mgs_ppl", 9)
    with pytest.raises(ValueError):
        gpu_ctx.set_option("mgs_ppl", 0)
    worst = {}
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        base = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12)
        _gm_ok(base, ref, TOL, tag)
        for opts in OPTION_SETTINGS:
            out = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12, **opts)
            _gm_ok(out, ref, TOL, (tag, opts))
            H_ok(out[4], base[4], 1e-12)
            worst[str(opts)] = max(_gm_dev(out, ref).values())
            if "mgs_fused" in opts:
                assert _bitwise(out, base), (tag, opts)
    print(f"[options {tag}] largest deviation from the oracle {max(worst.values()):.1e} ({max(worst, key=worst.get)})")


def _spreads(fn, A, nhist, seeds=range(1, 9)):
    """Per-entry spread of the oracle `fn(A)` = (x, hist...) under the rounding model: (ref, sx, [sh...])."""
    ref = fn(A)
    sx, sh = 0.0, [np.zeros(np.size(r_)) for r_ in ref[1:1 + nhist]]
    for seed in seeds:
        p = fn(_Rounded(A, np.random.default_rng(seed)))
        sx = max(sx, rel(p[0], ref[0]))
        for i in range(nhist):
            with np.errstate(invalid="ignore"):
                d = np.abs(np.asarray(p[1 + i]) - np.asarray(ref[1 + i])) / np.maximum(np.abs(ref[1 + i]), 1e-300)
            sh[i] = np.maximum(sh[i], np.nan_to_num(d))
    return ref, sx, sh


GKB = {"lsqr": (lambda AA, b, xt: R.lsqr_solver(AA, b, xt, 0.0, 12), hgmres.lsqr_solver, (), 2),
       "lsmr": (lambda AA, b, xt: R.lsmr_solver(AA, b, xt, 0.0, 12), hgmres.lsmr_solver, (), 3),
       "hybrid_lsqr": (lambda AA, b, xt: R.hybrid_lsqr_solver(AA, b, xt, 0.0, 12, LAM), hgmres.hybrid_lsqr_solver,
                       (LAM,), 2),
       "hybrid_lsmr": (lambda AA, b, xt: R.hybrid_lsmr_solver(AA, b, xt, 0.0, 12, LAM), hgmres.hybrid_lsmr_solver,
                       (LAM,), 2)}


@gpu
@pytest.mark.parametrize("solver", list(GKB))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_golub_kahan_odd_lengths(gpu_ctx, shape, solver):
    """fp64 LSQR / LSMR and their hybrids, 12 iterations, in test_gpu_parity._gkb_check's envelope (1e-10 floor,
    100x the oracle's own spread, 1e-6 cap).  At these inputs every history entry and x must come out judged
    under the cap: an envelope wider than 1e-6 would mean the input, not the kernel, decides the test."""
    A, B, b, xt = _problem(*shape)
    ofn, gfn, extra, nh = GKB[solver]
    fn = lambda AA: ofn(AA, b, xt)   # noqa: E731
    _, sx, sh = _spreads(fn, A, nh)
    assert 100.0 * sx <= GKB_CAP, ("x envelope past the cap", sx)
    for i in range(nh):
        assert np.all(100.0 * sh[i] <= GKB_CAP), ("history envelope past the cap", i, float(np.max(sh[i])))
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        out = gfn(Ao, b, xt, 0.0, 12, *extra, ctx=gpu_ctx, At=Bo)
    ref = _gkb_check(fn, A, out[:1 + nh], nhist=nh, label=f"{solver} {shape}")
    assert out[-1] == ref[-1] == 12


@gpu
@pytest.mark.parametrize("solver", ["lsqr", "lsmr"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_golub_kahan_fp32_odd_lengths(gpu_ctx, shape, solver):
    """LSQR / LSMR on an fp32 operator against the fp32 oracle on the same fp32 values, in the envelope of
    test_gpu_fused.test_fp32_one_pass_within_fp32_oracle_envelope: max(1e-6, 100x the oracle's spread over
    other fp32 summation orders (_Rounded32, 4 seeds)), x and every history entry."""
    A, B, b, xt = _problem(*shape)
    K, kfac = 12, 100.0
    A32 = sp.csr_matrix((A.data.astype(np.float32), A.indices, A.indptr), shape=A.shape)
    fn = {"lsqr": R.lsqr_solver_f32, "lsmr": R.lsmr_solver_f32}[solver]
    gfn = {"lsqr": hgmres.lsqr_solver, "lsmr": hgmres.lsmr_solver}[solver]
    nh = 2 if solver == "lsqr" else 3
    ref = fn(A32, b, xt, 0.0, K)
    sx, sh = 0.0, [np.zeros(K) for _ in range(nh)]
    for seed in range(1, 5):
        p = fn(_Rounded32(A32, np.random.default_rng(seed)), b, xt, 0.0, K)
        sx = max(sx, rel(p[0].astype(np.float64), ref[0].astype(np.float64)))
        for i in range(nh):
            sh[i] = np.maximum(sh[i], np.abs(p[1 + i] - ref[1 + i]) / np.abs(ref[1 + i]))
    with _device_ops(gpu_ctx, A32.astype(np.float64), A32.T.tocsr().astype(np.float64), dtype=L.HGM_F32) as (Ao, Bo):
        out = gfn(Ao, b, xt, 0.0, K, ctx=gpu_ctx, At=Bo)
    assert out[-1] == ref[-1] == K
    dx = rel(out[0], ref[0].astype(np.float64))
    msg = []
    for i in range(nh):
        d = np.abs(np.asarray(out[1 + i]) - ref[1 + i]) / np.abs(ref[1 + i])
        tol = np.maximum(1e-6, kfac * sh[i])
        msg.append(f"max dev {np.max(d):.1e}, {np.max(d / tol):.3f} of the bar")
        assert np.all(d <= tol), (i, float(np.max(d / tol)))
    print(f"[fp32 {solver} {shape}] x dev {dx:.2e} (oracle spread {sx:.2e}); histories: " + "; ".join(msg))
    assert dx <= max(1e-6, kfac * sx), (dx, sx)


# ---------------------------------------------------------------------------------------------
# 5. long runs: across step 120
# ---------------------------------------------------------------------------------------------
LONG_K = (120, 121, 124)
LONG_FROM = 118                 # columns / iterations from here on must be judged under the cap
# What the oracle's own spread supports at these shapes, measured on the CPU (8 seeds, k = 124, lambda = LAM;
# largest over the two shapes): the four bounds families H <= 3.7e-12, x <= 2.3e-11, histories <= 1.9e-11;
# hybrid_ba_gmres_rtp H 2.4e-11, x 4.7e-12, histories 2.9e-12.  Every envelope stays under the cap, so every
# entry is judged.  hybrid_ab_gmres_rtp (spread 1.4e-10; a 124-step oracle run of it takes over a second at
# 4097^2, nine of them per case) is not run here: its n-space sweep is hybrid_ba_gmres_rtp's.
LONG_ASSERTED = {tag: ("H", "x", "err", "res") for tag in ("abn", "abp", "bap", "ban", "hba")}
AB_BOUNDS = ("abn", "abp")


@contextlib.contextmanager
def _recorded_gemv():
    """The oracle forms each iteration's z_k = Q y_k by one call of its _gemv: keep them, so that one
    124-iteration run also gives the solutions a budget of 120 or 121 would have returned."""
    zs, orig = [], R._gemv

    def rec(Q, y):
        z = orig(Q, y)
        zs.append(z)
        return z
    R._gemv = rec
    try:
        yield zs
    finally:
        R._gemv = orig


def _oracle_long(tag, A, B, Bx, b, xt):
    """One oracle run of max(LONG_K) iterations: H, both histories and x after each budget of LONG_K (a
    shorter budget runs the same iterations; x = B*z on the AB side, with the unperturbed Bx)."""
    K = max(LONG_K)
    with _recorded_gemv() as zs:
        o = _gm_ref(tag, A, B, b, xt, K)
    assert o[3] == K and len(zs) == K
    xs = {k: (Bx @ zs[k - 1] if tag in AB_BOUNDS else zs[k - 1]) for k in LONG_K}
    assert np.array_equal(xs[K], o[0]) or tag in AB_BOUNDS
    return dict(H=o[4], err=o[1], res=o[2], x=xs)


def _ulp_copy(M, rng):
    """The operator with every value moved by at most one ulp (for B*A formed explicitly, which the
    rounding model cannot enter)."""
    Mp = M.copy()
    Mp.data = Mp.data * (1.0 + 2.220446049250313e-16 * rng.integers(-1, 2, Mp.data.size))
    return Mp


@functools.lru_cache(maxsize=None)
def _long_envelope(shape, tag):
    """Reference and tolerances max(1e-10, 100 x the oracle's spread under 8 seeds), per quantity and per
    entry (H against max|H|, x in norm per budget, histories relative), not yet capped."""
    A, B, b, xt = _problem(*shape)
    ref = _oracle_long(tag, A, B, B, b, xt)
    hmax = np.max(np.abs(ref["H"]))
    s = dict(H=np.zeros_like(ref["H"]), err=np.zeros(max(LONG_K)), res=np.zeros(max(LONG_K)),
             x={k: 0.0 for k in LONG_K})
    for seed in range(1, 9):
        rng = np.random.default_rng(seed)
        if tag == "ban":
            Ap = _ulp_copy(A, rng)
            p = _oracle_long(tag, Ap, Ap.T.tocsr(), B, b, xt)
        else:
            Ar = _Rounded(A, rng)
            p = _oracle_long(tag, Ar, Ar.T, B, b, xt)
        s["H"] = np.maximum(s["H"], np.abs(p["H"] - ref["H"]) / hmax)
        for h in ("err", "res"):
            s[h] = np.maximum(s[h], np.abs(p[h] - ref[h]) / np.abs(ref[h]))
        for k in LONG_K:
            s["x"][k] = max(s["x"][k], rel(p["x"][k], ref["x"][k]))
    tol = dict(H=np.maximum(TOL, 100.0 * s["H"]), err=np.maximum(TOL, 100.0 * s["err"]),
               res=np.maximum(TOL, 100.0 * s["res"]), x={k: max(TOL, 100.0 * v) for k, v in s["x"].items()})
    return ref, tol, s


def _long_check(out, ref, tol, K, what, label):
    """A K-iteration device solve inside the envelope.  Entries whose envelope exceeds the cap are not judged;
    from column / iteration LONG_FROM on every entry must be judged, or the test fails."""
    x, err, res, k, H = out
    assert k == K, (label, k)
    msg = []
    if "H" in what:
        Hr, tH = ref["H"][:K + 1, :K], tol["H"][:K + 1, :K]
        judged = tH <= GKB_CAP
        assert np.all(judged[:, LONG_FROM:]), (label, "H envelope past the cap across the hand-over")
        d = np.abs(H - Hr) / np.max(np.abs(ref["H"]))
        assert np.all(d[judged] <= tH[judged]), (label, "H", float(np.max(d[judged] / tH[judged])))
        msg.append(f"H {np.max(d[judged]):.1e} ({np.max(d[judged] / tH[judged]):.2f} of the bar, "
                   f"{int((~judged).sum())} entries past the cap)")
    for name, a, r_ in (("err", err, ref["err"][:K]), ("res", res, ref["res"][:K])):
        if name in what:
            t = tol[name][:K]
            judged = t <= GKB_CAP
            assert np.all(judged[LONG_FROM:]), (label, name, "envelope past the cap across the hand-over")
            d = np.abs(a - r_) / np.abs(r_)
            assert np.all(d[judged] <= t[judged]), (label, name, float(np.max(d[judged] / t[judged])))
            msg.append(f"{name} {np.max(d[judged]):.1e} ({np.max(d[judged] / t[judged]):.2f}, "
                       f"{int((~judged).sum())} past the cap)")
    if "x" in what:
        assert tol["x"][K] <= GKB_CAP, (label, "x envelope past the cap", tol["x"][K])
        dx = rel(x, ref["x"][K])
        assert dx <= tol["x"][K], (label, "x", dx, tol["x"][K])
        msg.append(f"x {dx:.1e} (bar {tol['x'][K]:.1e})")
    print(f"[long {label}] " + "; ".join(msg))


@gpu
@pytest.mark.parametrize("tag", list(LONG_ASSERTED))
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_runs_across_step_120(gpu_ctx, shape, tag):
    """Budgets 120 (the last that keeps the Gram monitor), 121 and 124: under the default mgs_single the padded
    one-workgroup kernel carries all steps; under mgs_single = 0 the one-reduction sweep hands over to the pass
    form at step 120, the pending normalisation is cut at kk + 2 <= 120 and the ring copy takes its other
    branch."""
    A, B, b, xt = _problem(*shape)
    ref, tol, _ = _long_envelope(shape, tag)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        for single in (1, 0):
            for K in LONG_K:
                out = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, K, mgs_single=single)
                _long_check(out, ref, tol, K, LONG_ASSERTED[tag], f"{tag} {shape} mgs_single={single} k={K}")


@gpu
@pytest.mark.parametrize("tag", list(GM))
@pytest.mark.parametrize("shape", LONG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_runs_bitwise(gpu_ctx, shape, tag):
    """mgs_single = 0.  Reproducibility: a 124-iteration solve repeated is bitwise equal in x, H and the
    histories (every sum has a fixed order).  Prefix equality: with gram_err = 0 the first 120 iterations of the
    124-iteration solve are bitwise those of the 120-iteration solve -- the budget changes only buffer strides,
    so a difference here points at the hand-over."""
    A, B, b, xt = _problem(*shape)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        a1 = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 124, mgs_single=0)
        a2 = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 124, mgs_single=0)
        l4 = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 124, mgs_single=0, gram_err=0)
        l0 = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 120, mgs_single=0, gram_err=0)
    assert _bitwise(a1, a2), tag
    assert l4[3] == 124 and l0[3] == 120
    assert np.array_equal(l4[4][:121, :120], l0[4]), tag
    assert np.array_equal(l4[1][:120], l0[1]) and np.array_equal(l4[2][:120], l0[2]), tag


# ---------------------------------------------------------------------------------------------
# 6. the pipeline and hand-over options at a small size
# ---------------------------------------------------------------------------------------------
BITWISE_OPTIONS = ([dict(pipe_depth=d) for d in range(1, 7)] + [dict(recon_serial=0), dict(recon_serial=1),
                   dict(recon_serial=-1, recon_serial_n=1), dict(sync_event_fence=0), dict(sync_event_fence=1)])


@gpu
@pytest.mark.parametrize("stop", [False, True], ids=["tol0", "stop5"])
@pytest.mark.parametrize("tag", ["hba", "abn"])
def test_pipeline_options_small(gpu_ctx, tag, stop):
    """1537 x 4097, 12 iterations, with tol = 0 and with a tol that stops at iteration 5 (speculative steps past
    it write no output).  pipe_depth, recon_serial(_n) and sync_event_fence change streams and events only, not
    kernels or summation orders: x, H, both histories and niters bitwise equal to the default.
    ring_poll = 0 forms beta = norm(r0) with the one-launch reduction and the host's sqrt where the default sums
    block partials and takes the square root on the device (normalize_to), and switches the Gram error
    monitor off: the sums are grouped differently, so the oracle at 1e-10 and the default at 1e-12 (measured:
    bitwise equal at this shape all the same, which is printed and not asserted).  krylov_pad pads only a
    leading dimension that is a multiple of 4096 and not padded for the one-workgroup sweep: none at this
    shape (held bitwise); a Krylov dimension of 4096 under mgs_single = 0 has one (1e-10 / 1e-12; measured
    bitwise equal, printed).  krylov_pad takes -1 or a multiple of 64: 2 is refused."""
    A, B, b, xt = _problem(*SMALL)
    tol = 0.0
    if stop:
        tol = float(_gm_ref(tag, A, B, b, xt, 12)[2][4]) * (1 + 1e-9)
    ref = _gm_ref(tag, A, B, b, xt, 12, tol)
    assert ref[3] == (5 if stop else 12)
    with pytest.raises(ValueError):
        gpu_ctx.set_option("krylov_pad", 2)
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        base = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12, tol)
        _gm_ok(base, ref, TOL, tag)
        for opts in BITWISE_OPTIONS + [dict(krylov_pad=64)]:
            out = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12, tol, **opts)
            assert _bitwise(out, base), (tag, opts)
        out = _gm_gpu(gpu_ctx, tag, Ao, Bo, b, xt, 12, tol, ring_poll=0)
        _gm_ok(out, ref, TOL, (tag, "ring_poll=0"))
        _gm_ok(out, base, 1e-12, (tag, "ring_poll=0 vs default"))
        print(f"[pipeline {tag} stop={stop}] ring_poll=0 bitwise equal to the default: {_bitwise(out, base)}")
    A2, B2, b2, xt2 = _problem(SMALL[0], 4096) if tag == "hba" else _problem(4096, SMALL[0])
    ref2 = _gm_ref(tag, A2, B2, b2, xt2, 12)
    with _device_ops(gpu_ctx, A2, B2) as (Ao, Bo):
        base2 = _gm_gpu(gpu_ctx, tag, Ao, Bo, b2, xt2, 12, mgs_single=0)
        pad = _gm_gpu(gpu_ctx, tag, Ao, Bo, b2, xt2, 12, mgs_single=0, krylov_pad=64)
    _gm_ok(pad, ref2, TOL, (tag, "krylov_pad=64"))
    _gm_ok(pad, base2, 1e-12, (tag, "krylov_pad=64 vs default"))
    print(f"[pipeline {tag}] krylov_pad=64 at dimension 4096 bitwise equal to the default: {_bitwise(pad, base2)}")


# ---------------------------------------------------------------------------------------------
# 7. device pointers on one context
# ---------------------------------------------------------------------------------------------
EX = {"abn": ("hgm_gmres_bounds_ex", (0.0, L.HGM_SIDE_AB, 0)), "bap": ("hgm_gmres_bounds_ex", (LAM, L.HGM_SIDE_BA, 1)),
      "hba": ("hgm_hybrid_ba_gmres_rtp_ex", (LAM,))}


def _ex_call(ctx, tag, Ao, Bo, b, xt, x, maxit, device):
    """One *_ex call: b, xt, x are numpy arrays (host pointers) or torch tensors (HGM_DEVICE_PTRS).  Returns
    (rc, err, res, niters, H)."""
    name, extra = EX[tag]
    ptr = (lambda t: C.cast(C.c_void_p(t.data_ptr()), L.dp)) if device else (lambda a: a.ctypes.data_as(L.dp))
    err, res, H, it = np.zeros(maxit), np.zeros(maxit), np.zeros((maxit + 1) * maxit), C.c_int(0)
    o = L.hgm_opts()
    o.flags, o.orth, o.H_out = (L.HGM_DEVICE_PTRS if device else 0), L.HGM_MGS, H.ctypes.data_as(L.dp)
    rc = getattr(L.load(), name)(ctx.handle, C.byref(o), Ao._h, Bo._h, ptr(b), ptr(xt), 0.0, maxit, *extra, ptr(x),
                                 err.ctypes.data_as(L.dp), res.ctypes.data_as(L.dp), C.byref(it))
    return rc, err[:it.value].copy(), res[:it.value].copy(), it.value, H


@gpu
@pytest.mark.parametrize("ring_poll", [1, 0])
@pytest.mark.parametrize("tag", list(EX))
def test_device_pointers_single_context(gpu_ctx, tag, ring_poll):
    """HGM_DEVICE_PTRS without a communicator (how the benchmark hands its vectors over): with ring_poll = 1
    the set-up norms are formed on the auxiliary stream and read from the ring at iteration 0.  The inputs are
    the same bytes and the norms have one summation order either way: x, H, the histories and niters bitwise
    equal to the host-pointer call."""
    import torch
    A, B, b, xt = _problem(*SMALL)
    dev = torch.device("cuda", 0)
    b_d, xt_d = torch.from_numpy(b).to(dev), torch.from_numpy(xt).to(dev)
    x_d = torch.zeros(A.shape[1], dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    x_h = np.zeros(A.shape[1])
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo), gpu_ctx.options(ring_poll=ring_poll):
        host = _ex_call(gpu_ctx, tag, Ao, Bo, b, xt, x_h, 12, False)
        devo = _ex_call(gpu_ctx, tag, Ao, Bo, b_d, xt_d, x_d, 12, True)
    assert host[0] == 0 and devo[0] == 0 and host[3] == devo[3] == 12
    assert np.array_equal(x_d.cpu().numpy(), x_h) and np.any(x_h != 0)
    for i in (1, 2, 4):
        assert np.array_equal(host[i], devo[i]), (tag, i)


@gpu
def test_device_pointers_must_be_16_byte_aligned(gpu_ctx):
    """The kernels read b and x_true in place as 16-byte pairs (gemv_rows), so include/hgmres.h requires
    16-byte alignment at HGM_DEVICE_PTRS: a view at an 8-byte offset into a larger tensor is refused with
    HGM_E_ARG, whichever of b, x_true and x it is, before any kernel runs."""
    import torch
    A, B, b, xt = _problem(*SMALL)
    m, n = A.shape
    dev = torch.device("cuda", 0)
    b_d, xt_d = torch.from_numpy(b).to(dev), torch.from_numpy(xt).to(dev)
    x_d = torch.zeros(n, dtype=torch.float64, device=dev)
    off = {k: torch.zeros(sz + 2, dtype=torch.float64, device=dev)[1:1 + sz] for k, sz in (("b", m), ("xt", n), ("x", n))}
    torch.cuda.synchronize()
    assert all(t.data_ptr() % 16 == 8 for t in off.values()) and b_d.data_ptr() % 16 == 0
    with _device_ops(gpu_ctx, A, B) as (Ao, Bo):
        for tag in EX:
            for which in off:
                args = dict(b=b_d, xt=xt_d, x=x_d)
                args[which] = off[which]
                rc, _, _, it, _ = _ex_call(gpu_ctx, tag, Ao, Bo, args["b"], args["xt"], args["x"], 12, True)
                assert rc == L.HGM_E_ARG and it == 0, (tag, which, rc)
        assert _ex_call(gpu_ctx, "hba", Ao, Bo, b_d, xt_d, x_d, 12, True)[0] == 0
