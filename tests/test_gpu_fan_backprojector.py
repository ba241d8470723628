"""The unmatched fan-beam back-projector on the device (hgm_mat_create_fan_backprojector, csrc/ops.hip
k_fan_backproj): with hgm_mat_create_fanbeam it is the problem class of run_2D_phantom.m:12-15, a curved-detector
fan beam whose back-projector is not A'.

* The generator against its numpy twin (hgmres.problems.fan_pixel_backprojector), bit for bit: indptr, indices
  and data, fp64 and fp32 (data against float32(w)), reference and tiled row order, a non-default span with
  det_offset = 0, and R = 0.75.  The kernel finds the bracketing rays from an atan2 guess that it verifies on
  the computed signs; the twin bisects (tests/test_fan_backprojector_cpu.py asserts the monotonicity that makes
  the two agree).
* Refusals (HGM_E_ARG).
* Every GMRES variant and both GCV Arnoldis on the unmatched pair at 32^2/90 (run_2D_phantom.m's own size),
  noise 1e-2, seed 0, k = 20, lambda = 1e-2, tol = 0, against the oracle restatement: H, x and both histories,
  on the device-generated tiled pair and on the host-uploaded CSR.  The bar of each quantity is
  max(1e-10, 100 x the oracle's own spread under test_gpu_parity._Rounded, 8 seeds), computed here.  Spreads
  measured on the CPU (largest entry; H against max|H|, x in norm, histories relative):
      hybrid_ab_gmres_rtp        H 9.4e-13  x 1.1e-13  hist 7.0e-13
      hybrid_ba_gmres_rtp        H 8.7e-13  x 1.0e-13  hist 4.2e-13
      ABgmres_hybrid_bounds      H 3.0e-13  x 4.5e-14  hist 1.9e-13
      ABgmres_nonhybrid_bounds   H 3.0e-13  x 2.2e-14  hist 1.6e-13
      BAgmres_hybrid_bounds      H 4.6e-13  x 1.1e-13  hist 3.5e-13
      BAgmres_nonhybrid_bounds   H 1.2e-13  x 2.1e-14  hist 6.6e-14   (see below)
      arnoldi ab                 H 3.9e-13             arnoldi ba   H 1.15e-12
  so every bar is 1e-10 but the BA Arnoldi's H (1.15e-10).  BAgmres_nonhybrid_bounds forms B*A explicitly
  (BAgmres_nonhybrid_bounds.m:4), which the rounding model of a product with a vector cannot enter: its spread
  is measured with the project's model for that case, a copy of A and B with every value moved by at most one
  ulp (test_gpu_lengths._ulp_copy, restated here), 8 seeds.
* The lockstep mismatch sweep on the general-pattern branch of k_spmm_pert: B0 = A', E = B_fan - A' built on the
  host (184,326 entries on the union of the two patterns against the 117,934 of B0), coefs 0 .. 1, ABgmres_nonhybrid_bounds and
  BAgmres_hybrid_bounds at k = 12, each level against the oracle on B0 + c E formed in scipy at the same kind
  of bar (oracle spreads measured on the CPU: at most 4.4e-13, so 1e-10), the level c = 1 against the oracle on
  (A, B_fan) itself.
* B.row_slice over whole tile columns (the pixel shards of hgmres.dist) equals the twin's rows in stored order.

LSQR / LSMR do not use B and are not run here.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres.core import stored_pixel_index
from hgmres.dist import tile_column_shards
from hgmres.problems import FAN_R, fan_pixel_backprojector, tomo_problem
from oracle import restatement as R   # checker only
from test_gpu_parity import _Rounded

pytestmark = pytest.mark.gpu

TOL = 1e-10
N0, NA0, K, LAM = 32, 90, 20, 1e-2
K_SWEEP = 12
COEFS = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
SOLVERS = {"hab": ("hybrid_ab_gmres_rtp", (LAM,)), "hba": ("hybrid_ba_gmres_rtp", (LAM,)),
           "abp": ("ABgmres_hybrid_bounds", (LAM,)), "abn": ("ABgmres_nonhybrid_bounds", ()),
           "bap": ("BAgmres_hybrid_bounds", (LAM,)), "ban": ("BAgmres_nonhybrid_bounds", ())}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


def _ulp_copy(M, rng):
    """The operator with every value moved by at most one ulp (test_gpu_lengths._ulp_copy)."""
    Mp = M.copy()
    Mp.data = Mp.data * (1.0 + 2.220446049250313e-16 * rng.integers(-1, 2, Mp.data.size))
    return Mp


# ---------------------------------------------------------------------------------------------
# 1. the generator, bit for bit
# ---------------------------------------------------------------------------------------------
def _same_bits(Bd, ref, dtype):
    M = Bd.to_scipy()                 # reference pixel order, values as float64
    assert Bd.shape == ref.shape and Bd.nnz == ref.nnz, (Bd.shape, Bd.nnz, ref.shape, ref.nnz)
    assert np.array_equal(M.indptr, ref.indptr)
    assert np.array_equal(M.indices, ref.indices)
    want = ref.data if dtype == L.HGM_F64 else ref.data.astype(np.float32).astype(np.float64)
    assert np.array_equal(M.data, want)


@pytest.mark.parametrize("N,na", [(1, 1), (2, 3), (32, 90), (64, 90), (48, 37)])
@pytest.mark.parametrize("order", ["reference", "auto"])
def test_fan_backprojector_device_generator_bitwise(gpu_ctx, N, na, order):
    ref = fan_pixel_backprojector(N, na)
    for dt in (L.HGM_F64, L.HGM_F32):
        B = hgmres.SparseOperator.fan_backprojector(N, na, ctx=gpu_ctx, dtype=dt, order=order)
        if order == "auto" and N % 4 == 0:
            assert B.pixel_order("rows") == (N, 4, 0)
        _same_bits(B, ref, dt)
        B.close()


@pytest.mark.parametrize("kw", [dict(span=0.45, det_offset=0.0), dict(R=0.75), dict(R=0.75, span=1.1, det_offset=0.0)],
                         ids=["span-nooffset", "R0.75", "R0.75-span-nooffset"])
def test_fan_backprojector_device_generator_geometry_arguments(gpu_ctx, kw):
    """A narrower fan than the image (pixels outside it drop their pairs) without the quarter offset, and a
    source just outside the image, where the fan angle of a pixel varies fastest."""
    N, na = 48, 37
    tw = dict(R=kw.get("R", FAN_R), span=kw.get("span"))
    if "det_offset" in kw:
        tw["det_offset"] = kw["det_offset"]
    ref = fan_pixel_backprojector(N, na, **tw)
    if "span" in kw:
        assert ref.nnz < fan_pixel_backprojector(N, na, R=tw["R"]).nnz       # the narrower fan loses pairs
    for order in ("reference", "auto"):
        for dt in (L.HGM_F64, L.HGM_F32):
            B = hgmres.SparseOperator.fan_backprojector(N, na, ctx=gpu_ctx, dtype=dt, order=order, **kw)
            _same_bits(B, ref, dt)
            B.close()


def test_fan_backprojector_refusals(gpu_ctx):
    import ctypes as C
    lib = L.load()

    def make(N, na, R=2.0, span=0.0, off=0.25, tile=1, sup=0):
        h = C.c_void_p()
        rc = lib.hgm_mat_create_fan_backprojector(gpu_ctx.handle, N, na, R, span, off, L.HGM_F64, tile, sup, C.byref(h))
        if rc == L.HGM_OK:
            lib.hgm_mat_destroy(h)
        else:
            assert not h.value
        return rc

    assert make(8, 4) == L.HGM_OK
    assert make(0, 4) == L.HGM_E_ARG and make(-8, 4) == L.HGM_E_ARG          # N <= 0
    assert make(8, 0) == L.HGM_E_ARG
    assert make(8, 4, R=1.0 / np.sqrt(2.0)) == L.HGM_E_ARG                   # R <= 1/sqrt(2)
    assert make(8, 4, R=0.5) == L.HGM_E_ARG
    assert make(8, 4, span=np.pi) == L.HGM_E_ARG and make(8, 4, span=4.0) == L.HGM_E_ARG   # span >= pi
    assert make(8, 4, tile=3) == L.HGM_E_ARG                                 # a tile that does not divide N
    assert make(8, 4, tile=2, sup=3) == L.HGM_E_ARG
    assert lib.hgm_mat_create_fan_backprojector(gpu_ctx.handle, 8, 4, 2.0, 0.0, 0.25, L.HGM_F64, 1, 0, None) == L.HGM_E_ARG
    assert make(8, 4, tile=4) == L.HGM_OK                                    # the context still works


# ---------------------------------------------------------------------------------------------
# 2. the solvers on the unmatched pair
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _problem():
    P = tomo_problem(N0, NA0, noise=1e-2, seed=0, backprojector="fanpixel", geometry_kind="fan")
    P.b.setflags(write=False)
    P.x_true.setflags(write=False)
    return P


@pytest.fixture(scope="module")
def pairs(gpu_ctx):
    P = _problem()
    A = hgmres.SparseOperator.fanbeam(N0, NA0, ctx=gpu_ctx)                  # tiled pixel order (production)
    B = hgmres.SparseOperator.fan_backprojector(N0, NA0, ctx=gpu_ctx)
    assert A.pixel_order("cols") == B.pixel_order("rows") == (N0, 4, 0)
    Ah = hgmres.SparseOperator.from_scipy(P.A, gpu_ctx)
    Bh = hgmres.SparseOperator.from_scipy(P.B, gpu_ctx)
    try:
        info = hgmres.fused_plan_info(A, B)
        print(f"[fan unmatched {N0}^2/{NA0}] one-pass plan accepted: {info['nslot']} slots")
    except (ValueError, hgmres.HgmError) as e:
        print(f"[fan unmatched {N0}^2/{NA0}] one-pass plan refused ({e}): two-pass path")
    yield {"tiled": (A, B), "host": (Ah, Bh)}
    for M in (A, B, Ah, Bh):
        M.close()


def _quantities(o):
    """(H, x, err, res) of a solver's (x, err, res, niters, ..., H)."""
    return dict(H=np.asarray(o[-1]), x=np.asarray(o[0]), err=np.asarray(o[1]), res=np.asarray(o[2]))


def _dev(got, ref):
    return dict(H=float(np.max(np.abs(got["H"] - ref["H"])) / np.max(np.abs(ref["H"]))), x=rel(got["x"], ref["x"]),
                err=float(np.max(np.abs(got["err"] - ref["err"]) / np.abs(ref["err"]))),
                res=float(np.max(np.abs(got["res"] - ref["res"]) / np.abs(ref["res"]))))


def _bars(run, A, B, explicit=False):
    """The oracle's result and max(TOL, 100 x its spread) per quantity: 8 seeds of the rounding model on both
    operators, or of the 1-ulp copy where the oracle forms B*A explicitly."""
    ref = _quantities(run(A, B))
    spread = dict.fromkeys(ref, 0.0)
    for seed in range(1, 9):
        rng = np.random.default_rng(seed)
        Ap, Bp = (_ulp_copy(A, rng), _ulp_copy(B, rng)) if explicit else (_Rounded(A, rng), _Rounded(B, rng))
        d = _dev(_quantities(run(Ap, Bp)), ref)
        spread = {q: max(spread[q], d[q]) for q in spread}
    return ref, {q: max(TOL, 100.0 * s) for q, s in spread.items()}, spread


def _judge(tag, dev, bar, spread):
    print(f"[fan unmatched {tag}] " + " ".join(f"{q}: dev {dev[q]:.2e} bar {bar[q]:.2e} (spread {spread[q]:.1e})"
                                                for q in dev))
    for q in dev:
        assert dev[q] <= bar[q], (tag, q, dev[q], bar[q])


@pytest.mark.parametrize("name", list(SOLVERS))
def test_gmres_variants_on_the_unmatched_fan_pair(gpu_ctx, pairs, name):
    P = _problem()
    fn, args = SOLVERS[name]
    run = lambda A, B: getattr(R, fn)(A, B, P.b, P.x_true, 0.0, K, *args, return_H=True)   # noqa: E731
    ref, bar, spread = _bars(run, P.A, P.B, explicit=(name == "ban"))
    for tag, (Ao, Bo) in pairs.items():
        o = getattr(hgmres, fn)(Ao, Bo, P.b, P.x_true, 0.0, K, *args, ctx=gpu_ctx, return_H=True)
        assert o[3] == K
        _judge(f"{tag} {name}", _dev(_quantities(o), ref), bar, spread)


@pytest.mark.parametrize("typ", ["ab", "ba"])
def test_gcv_arnoldi_on_the_unmatched_fan_pair(gpu_ctx, pairs, typ):
    P = _problem()
    Hr, br = R.arnoldi(P.A, P.B, P.b, K, typ)
    sH = sb = 0.0
    for seed in range(1, 9):
        rng = np.random.default_rng(seed)
        Hp, bp = R.arnoldi(_Rounded(P.A, rng), _Rounded(P.B, rng), P.b, K, typ)
        sH = max(sH, float(np.max(np.abs(Hp - Hr)) / np.max(np.abs(Hr))))
        sb = max(sb, abs(bp - br) / br)
    bar_H, bar_b = max(TOL, 100.0 * sH), max(TOL, 100.0 * sb)
    for tag, (Ao, Bo) in pairs.items():
        H, beta, kd = hgmres.arnoldi(Ao, Bo, P.b, K, typ, ctx=gpu_ctx)
        dH = float(np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)))
        db = abs(beta - br) / br
        print(f"[fan unmatched {tag} arnoldi {typ}] H: dev {dH:.2e} bar {bar_H:.2e} (spread {sH:.1e}) "
              f"beta: dev {db:.2e} bar {bar_b:.2e} (spread {sb:.1e})")
        assert kd == K and dH <= bar_H and db <= bar_b


# ---------------------------------------------------------------------------------------------
# 3. the lockstep mismatch sweep from A' to the fan back-projector (general-pattern E)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side,hybrid", [("ab", False), ("ba", True)])
def test_mismatch_sweep_from_matched_to_fan_backprojector(gpu_ctx, side, hybrid):
    P = _problem()
    B0 = sp.csr_matrix(P.A.T)
    B0.sort_indices()
    E = sp.csr_matrix(P.B - B0)
    E.sort_indices()
    assert E.nnz > B0.nnz                                                   # not B0's pattern: the general branch
    fn = R.BAgmres_hybrid_bounds if hybrid else R.ABgmres_nonhybrid_bounds
    args = (LAM,) if hybrid else ()
    run = lambda A, B: fn(A, B, P.b, P.x_true, 0.0, K_SWEEP, *args, return_H=True)   # noqa: E731
    Ao, B0o, Eo = (hgmres.SparseOperator.from_scipy(M, gpu_ctx) for M in (P.A, B0, E))
    Rb = hgmres.gmres_bounds_mismatch(Ao, B0o, Eo, COEFS, P.b, P.x_true, 0.0, K_SWEEP, side,
                                      lambdas=np.full(COEFS.size, LAM) if hybrid else None, ctx=gpu_ctx, return_H=True)
    assert np.all(Rb.status == L.HGM_OK) and np.all(Rb.niters == K_SWEEP)
    for j, c in enumerate(COEFS):
        got = dict(H=Rb.H[j], x=Rb.x[:, j], err=Rb.error_norm[:, j], res=Rb.residual_norm[:, j])
        ref, bar, spread = _bars(run, P.A, sp.csr_matrix(B0 + c * E))
        _judge(f"sweep {side}{'p' if hybrid else 'n'} c={c}", _dev(got, ref), bar, spread)
    ref, bar, spread = _bars(run, P.A, P.B)                                 # c = 1 is the fan back-projector itself
    _judge(f"sweep {side}{'p' if hybrid else 'n'} c=1 vs B_fan", _dev(got, ref), bar, spread)
    for M in (Ao, B0o, Eo):
        M.close()


# ---------------------------------------------------------------------------------------------
# 4. pixel shards
# ---------------------------------------------------------------------------------------------
def test_row_slices_over_tile_columns_are_the_twins_rows_in_stored_order(gpu_ctx):
    N, na = 32, 90
    ref = sp.csr_matrix(_problem().B)
    B = hgmres.SparseOperator.fan_backprojector(N, na, ctx=gpu_ctx)
    Nn, tile, sup = B.pixel_order("rows")
    assert (Nn, tile, sup) == (N, 4, 0)
    ref_of_stored = np.argsort(stored_pixel_index(N, tile, sup))
    shards = tile_column_shards(N, 3, tile)                                 # 8 tile columns over 3 ranks: uneven
    assert shards[0][0] == 0 and shards[-1][1] == N * N and len({hi - lo for lo, hi in shards}) > 1
    for lo, hi in shards:
        assert lo % (tile * N) == 0 and hi % (tile * N) == 0
        S = B.row_slice(lo, hi)
        M = S.to_scipy()
        want = ref[ref_of_stored[lo:hi]]
        assert M.shape == want.shape == (hi - lo, ref.shape[1])
        assert np.array_equal(M.indptr, want.indptr) and np.array_equal(M.indices, want.indices)
        assert np.array_equal(M.data, want.data)
        S.close()
    B.close()
