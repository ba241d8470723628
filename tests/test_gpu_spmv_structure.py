"""The SpMV kernels and the operator builders at their structure edges (csrc/spmv.hip, csrc/ops.hip).

The matrices are those of spmv_cases.py, sized from the constants of csrc/:
  1. rows that end, start, vanish or stop on multiples of the streaming chunk SCH (who writes the row:
     `has_head`, `send > c1`, `fo[k]` of k_spmv_stream / k_stream_fixup / k_chunk_fo);
  2. rows of 0..3 and of 2G, 4G, 8G (+-1), 16G + 1 entries at both start parities (the head / tail peel and
     the loop steps of the paired-load row kernel seg_partial<VEC>);
  3. operators of 65535 / 65536 / 65537 columns with entries in columns 0, 32767, 32768, 65535 (and 65536):
     the 16-bit copy of the column indices (build_ci16);
  4. full chunks touching exactly PG_MAX, PG_MAX + 1 (fp64) and PG_MAX, PG_MAX + 1, 2 PG_MAX, 2 PG_MAX + 1
     (fp32) pages of x, and one touching the last, partial page (the paged gather's limits);
  5. 1 x n, m x 1, m x 2, 1 x 1, one non-empty last row, no entries;
  6. rows with shuffled and repeated columns.

Reference: the row sums over the CSR arrays in np.longdouble (exact fractions where long double is no
wider than fp64), from inputs rounded to the operator's type.  Bounds per row i of L_i entries,
s_i = (|M||x|)_i: |y_i - ref_i| <= gamma(L_i + 1) s_i with gamma(k) = k u / (1 - k u) (a dot product in any
summation order; u = 2^-53 / 2^-24), an empty row exactly 0, a one-entry row within one rounding, and in
fp64 the project's bar 1e-14 (s_i + 1e-300).  Every product runs twice (same bits) into a NaN-filled
output, so a row that no workgroup writes is seen.  Equal bits are asserted wherever the code promises
them: nontemporal loads and XCD order on / off, paged against unpaged streaming (paged16 on / off), 65536
against 65537 columns, bands at least as wide as the operator against none, an unaligned x, and every
builder against numpy / scipy.

What the code does with unsorted and repeated columns (case 6), read from create_csr_impl, k_band_fill,
k_page_index and transpose and pinned here: nothing sorts or merges.  The arrays are stored as given
(to_scipy returns them); every kernel multiplies entry by entry, so a repeated column adds twice; the band
builder keeps the stream order inside a band; the page index sorts (page, position) pairs of a chunk and
is indifferent to the order; the transpose is a stable sort by column, so an output row lists its entries
in the CSR stream order of the input, repeated ones included.  No path needs a refusal.

The largest ratios to the two bounds are printed by every test (run with -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from oracle import restatement as R   # checker only
import spmv_cases as SC
from test_gpu_parity import TOL, H_ok, hist_ok, rel

gpu = pytest.mark.gpu

K = SC.constants()
ROW_GROUPS, STREAM_GROUPS = K["ROW_GROUPS"], K["STREAM_GROUPS"]
SCH = K["SCH"]
NT, XCD, STREAM, PAGED = 2, 4, 8, 16
FT = {0: np.float64, 1: np.float32}
DTYPES = [pytest.param(0, id="f64"), pytest.param(1, id="f32")]


# ---------------------------------------------------------------------------------------------
# CPU: every case has the property it is named for
# ---------------------------------------------------------------------------------------------
def test_constants_read_from_csrc():
    assert SCH >= 1024 and SCH % 1024 == 0
    assert K["PG_BYTES"] == 128 and K["PG_MAX64"] * K["PG_BYTES"] >= SCH * 8
    assert K["PG_MAX32"] * K["PG_BYTES"] <= SCH * 4 and K["PG_ROUNDS32"] >= 1
    assert K["SPMV_U"] == 4 and K["CI16_MAX"] == 65536
    assert set(ROW_GROUPS) == {4, 8, 16, 32, 64} and set(STREAM_GROUPS) == {2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize("name,total,tail", [("chunk_multiple", 8 * SCH, 3), ("chunk_multiple_plus1", 8 * SCH + 1, 3)])
def test_case1_rows_sit_on_the_chunk_boundaries(name, total, tail):
    M, _ = SC.case(name)
    p, Ln = M.indptr, np.diff(M.indptr)
    lo, hi = p[:-1], p[1:]
    S = SCH
    assert M.shape[1] == SC.N_CHUNK and 50 <= M.shape[0] <= 70 and M.nnz == total
    assert M.has_canonical_format
    assert np.any((Ln > 0) & (hi == S)), "a row ending exactly at SCH"
    at = np.flatnonzero((Ln == 0) & (lo == S))
    assert at.size >= 3 and np.all(np.diff(at) == 1), "a run of empty rows whose pointer equals SCH"
    assert Ln[at[0] - 1] > 0 and Ln[at[-1] + 1] > 0
    assert np.any((lo == S) & (hi == 2 * S)), "a row of SCH entries occupying chunk [SCH, 2 SCH)"
    whole = hi // S - -(-lo // S)               # whole chunks inside the row
    assert np.any((lo % S != 0) & (hi % S != 0) & (whole >= 1) & (Ln > 2 * S)), "mid-chunk to mid-chunk over a chunk"
    assert np.any((lo % S != 0) & (hi % S == 0) & (Ln > 1)), "mid-chunk to a boundary"
    before = set((hi[(Ln == 1) & (hi % S == 0)] // S).tolist())
    after = set((lo[(Ln == 1) & (lo % S == 0)] // S).tolist())
    assert before & after, "single-entry rows on both sides of one boundary"
    assert Ln[0] == 0 and Ln[1] == 0 and np.all(Ln[-tail:] == 0) and Ln[-tail - 1] > 0
    if total % S:
        assert total % S == 1 and Ln[-tail - 1] == 1    # the last chunk holds one entry, a row of its own


def test_case1_small_totals():
    for name, total in (("chunk_minus1", SCH - 1), ("chunk_exact", SCH)):
        M, _ = SC.case(name)
        Ln = np.diff(M.indptr)
        assert M.nnz == total and Ln[0] == 0 and Ln[-1] == 0 and np.any(Ln == 1) and Ln.max() > 1000


def test_case2_lengths_and_parities():
    M, _ = SC.case("pairs")
    plan = SC.pair_plan()
    Ln, start = np.diff(M.indptr), M.indptr[:-1]
    assert M.shape == (len(plan), SC.N_PAIR) and 4 * K["SPMV_U"] * max(ROW_GROUPS) + 1 <= SC.N_PAIR
    seen = set()
    for r, (G, length, parity) in enumerate(plan):
        assert Ln[r] == length and start[r] % 2 == parity, (r, G, length, parity)
        if G:
            seen.add((G, length, parity))
    U = K["SPMV_U"]
    assert U == 4                                   # the loop steps below are 8G, 4G, 2G entries
    for G in ROW_GROUPS:
        want = [0, 1, 2, 3, 2 * G - 1, 2 * G, 2 * G + 1, 4 * G - 1, 4 * G + 1, 8 * G - 1, 8 * G, 8 * G + 1, 16 * G + 1]
        for length in want:
            for parity in (0, 1):
                assert (G, length, parity) in seen, (G, length, parity)


def test_case3_columns_around_the_16_bit_limit():
    lim = K["CI16_MAX"]
    base, _ = SC.case("width_ci16")
    plus, _ = SC.case("width_ci16_plus1")
    past, _ = SC.case("width_col_past16")
    minus, _ = SC.case("width_ci16_minus1")
    assert base.shape == (48, lim) and plus.shape == (48, lim + 1) and past.shape == (48, lim + 1)
    assert minus.shape == (48, lim - 1) and 13000 <= base.nnz <= 15000
    for a in ("indptr", "indices", "data"):
        assert np.array_equal(getattr(base, a), getattr(plus, a)), a
    assert np.array_equal(base.indptr, past.indptr) and np.array_equal(base.indptr, minus.indptr)
    for r in range(48):
        row = base.indices[base.indptr[r]:base.indptr[r + 1]]
        assert {0, lim // 2 - 1, lim // 2, lim - 1} <= set(row.tolist())
        prow = past.indices[past.indptr[r]:past.indptr[r + 1]]
        assert prow[-1] == lim and np.count_nonzero(prow == lim) == 1 and np.setdiff1d(row, prow).size == 1
        assert {0, lim // 2 - 1, lim // 2, lim - 1} <= set(prow.tolist())
        assert np.all(np.diff(prow) > 0)
        mrow = minus.indices[minus.indptr[r]:minus.indptr[r + 1]]
        assert mrow.max() == lim - 2 and np.all(np.diff(mrow) > 0)
    assert np.array_equal(np.sort(base.data), np.sort(past.data))


@pytest.mark.parametrize("name,es,counts", [("pages64", 8, SC.pages64_counts()), ("pages32", 4, SC.pages32_counts())])
def test_case4_chunks_touch_the_stated_page_counts(name, es, counts):
    M, _ = SC.case(name)
    E = K["PG_BYTES"] // es
    n = M.shape[1]
    got = SC.chunk_page_counts(M, E, SCH)
    assert got == counts + [100], (got, counts)
    pmax = K["PG_MAX64"] if es == 8 else K["PG_MAX32"]
    rounds = 1 if es == 8 else K["PG_ROUNDS32"]
    assert counts[0] == pmax and counts[-2] == rounds * pmax and counts[-1] == rounds * pmax + 1
    assert n % 32 and n % 16 and n - 1 in M.indices[len(counts) * SCH:(len(counts) + 1) * SCH]
    assert 0 < M.nnz % SCH < SCH and M.has_canonical_format     # a final partial chunk
    assert M.nnz <= 150000 and n <= 70000


def test_case5_shapes():
    want = {"one_row": ((1, 10000), 10000), "one_col": ((300, 1), None), "two_cols": ((9, 2), 9),
            "one_by_one": ((1, 1), 1), "last_row_only": ((200, 50), 37), "no_entries": ((4, 3), 0)}
    for name, (shape, nnz) in want.items():
        M, _ = SC.case(name)
        assert M.shape == shape and (nnz is None or M.nnz == nnz), name
    M, _ = SC.case("one_col")
    assert 100 < M.nnz < 200
    M, _ = SC.case("last_row_only")
    assert np.all(np.diff(M.indptr)[:-1] == 0)


def test_case6_is_unsorted_with_duplicates_and_scipy_left_it_alone():
    M, x = SC.case("unsorted")
    assert M.shape == (40, 9000) and 8000 <= M.nnz <= 12000
    assert M.tocsr() is M and not M.has_sorted_indices and not M.has_canonical_format
    counts = []
    for r in range(40):
        row = M.indices[M.indptr[r]:M.indptr[r + 1]]
        assert np.any(np.diff(row) < 0), r
        _, c = np.unique(row, return_counts=True)
        counts.append(sorted(c[c > 1].tolist()))
    assert counts.count([2, 3]) == 8 and counts.count([]) == 32
    # the reference over the stored entries is the reference of the matrix with duplicates summed
    if SC.WIDE_OK:
        for dtype in (0, 1):
            ref = SC.reference("unsorted", dtype)
            want, scale = SC.summed_dense_product(M, x, dtype)
            assert np.all(np.abs(ref.ref - want) <= 4 * ref.slack + 1e-300)
            assert np.all(scale.astype(np.float64) <= ref.s * (1 + 1e-12))


def test_reference_long_double_against_fractions():
    M, x = SC.case("last_row_only")
    rng = np.random.default_rng(3)
    for dtype in (0, 1):
        exact = SC.Reference(M, x, dtype, wide=False)
        y = np.array([float(v) for v in exact.ref]).astype(FT[dtype]).astype(np.float64)
        rd, _ = exact.check(y)
        assert rd <= 1.0
        bad = y.copy()
        bad[-1] += 64 * SC.UNIT[dtype] * exact.s[-1]
        with pytest.raises(AssertionError):
            exact.check(bad)
        if SC.WIDE_OK:
            wide = SC.Reference(M, x, dtype, wide=True)
            assert np.all(wide.errors(y) <= exact.errors(y) + wide.slack)
            wide.check(y)
            with pytest.raises(AssertionError):
                wide.check(bad)
            one = y.copy()
            one[0] = rng.standard_normal()              # an empty row must be exactly 0
            with pytest.raises(AssertionError):
                wide.check(one)


# --- the solver leg -------------------------------------------------------------------------
STEPS, LAM = 4, 1e-2
SOLVERS = {"ab": (hgmres.hybrid_ab_gmres_rtp, R.hybrid_ab_gmres_rtp),
           "ba": (hgmres.hybrid_ba_gmres_rtp, R.hybrid_ba_gmres_rtp)}


@functools.lru_cache(maxsize=None)
def _solver_problem():
    """A = case 1 (a multiple of SCH plus one entry), B = A' in the stable order, b = A x_true"""
    A, _ = SC.case("chunk_multiple_plus1")
    ip, ix, da = SC.stable_transpose(A)
    B = sp.csr_matrix((da, ix, ip), shape=(A.shape[1], A.shape[0]))
    xt = np.random.default_rng(99).standard_normal(A.shape[1])
    return A, B, A @ xt, xt


@functools.lru_cache(maxsize=None)
def _solver_oracle(tag):
    A, B, b, xt = _solver_problem()
    return SOLVERS[tag][1](A, B, b, xt, 0.0, STEPS, LAM, return_H=True)


@pytest.mark.parametrize("tag", sorted(SOLVERS))
def test_oracle_runs_the_solver_leg_to_its_last_step(tag):
    A, B, _, _ = _solver_problem()
    assert np.any(np.diff(B.indptr) == 0) and np.any(np.diff(A.indptr) == 0)   # empty rows meet the epilogues
    x, e, r, k, H = _solver_oracle(tag)
    assert k == STEPS and e.shape == r.shape == (STEPS,)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(e)) and np.all(np.isfinite(r)) and np.all(r > 0)
    sub = np.array([H[j + 1, j] for j in range(STEPS)])
    assert np.all(sub > 1e-8 * np.max(np.abs(H))), sub      # no breakdown, and none near


# ---------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------
class _Dev:
    """x of one operator on the device, aligned and (behind a one-element lead-in) advanced by one
    element, and an output buffer that is filled with NaN before every product."""

    def __init__(self, ctx, op, x):
        self.ctx, self.op, self.lib = ctx, op, L.load()
        self.ft = FT[op.dtype]
        self.es = np.dtype(self.ft).itemsize
        xs = np.ascontiguousarray(x, dtype=self.ft)
        assert xs.size == op.shape[1]
        self.ptrs = []
        self.x = self._upload(xs)
        self.xlead = self._upload(np.concatenate([np.full(1, 3.0, self.ft), xs]))
        self.nan = np.full(max(1, op.shape[0]), np.nan, dtype=self.ft)
        self.y = self._upload(self.nan)

    def _upload(self, a):
        p = C.c_void_p()
        assert self.lib.hgm_dev_alloc(self.ctx.handle, self.es * max(1, a.size), C.byref(p)) == L.HGM_OK
        self.ptrs.append(p)
        assert self.lib.hgm_memcpy_h2d(self.ctx.handle, p, a.ctypes.data_as(C.c_void_p), self.es * a.size) == L.HGM_OK
        return p

    def product(self, op=None, unaligned=False):
        op = op or self.op
        rows = op.shape[0]
        assert rows <= self.nan.size
        assert self.lib.hgm_memcpy_h2d(self.ctx.handle, self.y, self.nan.ctypes.data_as(C.c_void_p),
                                       self.es * self.nan.size) == L.HGM_OK
        xp = self.xlead.value + self.es if unaligned else self.x.value
        assert (xp % 16 != 0) == bool(unaligned)
        op.matvec_device(xp, self.y.value)
        out = np.empty(self.nan.size, dtype=self.ft)
        assert self.lib.hgm_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), self.y,
                                       self.es * out.size) == L.HGM_OK
        assert np.all(np.isnan(out[rows:])) or rows == 0
        return out[:rows].astype(np.float64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            if p.value:
                self.lib.hgm_dev_free(self.ctx.handle, p)
        return False


class _Worst:
    """largest ratios to the derived and to the 1e-14 bound over the products of one test"""

    def __init__(self, label):
        self.label, self.rd, self.rp, self.n = label, 0.0, float("nan"), 0

    def add(self, ratios):
        self.rd = max(self.rd, ratios[0])
        if not np.isnan(ratios[1]):
            self.rp = ratios[1] if np.isnan(self.rp) else max(self.rp, ratios[1])
        self.n += 1

    def report(self):
        print(f"RATIO {self.label}: {self.n} products, largest |y-ref| / derived bound {self.rd:.3f}, "
              f"/ (1e-14 s) {self.rp:.3f}")


def _twice(dev, ref, worst, what, **kw):
    y = dev.product(**kw)
    assert np.array_equal(y, dev.product(**kw)), (what, "not reproducible")
    worst.add(ref.check(y, what))
    return y


def _transpose(ctx, op):
    """a fresh device transpose (SparseOperator.T caches, and hands the original back for .T.T)"""
    h = C.c_void_p()
    rc = L.load().hgm_mat_transpose(ctx.handle, op._h, C.byref(h))
    assert rc == L.HGM_OK, rc
    return hgmres.SparseOperator._wrap(ctx, h)


def _rounded(data, dtype):
    return data.astype(np.float32).astype(np.float64) if dtype == 1 else data


def _same_csr(got, indptr, indices, data, dtype, what):
    assert np.array_equal(got.indptr, indptr), (what, "indptr")
    assert np.array_equal(got.indices, indices), (what, "indices")
    if dtype == 1:
        assert np.array_equal(got.data.astype(np.float32), np.asarray(data).astype(np.float32)), (what, "data")
    else:
        assert np.array_equal(got.data, data), (what, "data")


# ---------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_products_at_every_variant_and_lane_count(gpu_ctx, name, dtype):
    """Row-kernel variants 0-7 at every lane count of RowGroups, streaming 8, 8|2, 8|4, 8|16, 8|2|16 at
    every lane count of StreamGroups: the reference bounds, and equal bits for nontemporal / XCD on and
    off, and for paged against unpaged (paged16 on and off where the indices are narrowed)."""
    M, x = SC.case(name)
    ref = SC.reference(name, dtype)
    worst = _Worst(f"products {name} {FT[dtype].__name__}")
    op = hgmres.SparseOperator.from_scipy(M, gpu_ctx, dtype=dtype)
    try:
        with _Dev(gpu_ctx, op, x) as dev:
            for g in ROW_GROUPS:
                ys = {}
                for v in range(8):
                    op.tune(v, g)
                    ys[v] = _twice(dev, ref, worst, (name, dtype, v, g))
                for v in (NT, XCD, NT | XCD):
                    assert np.array_equal(ys[v], ys[0]), (name, dtype, v, g)
                    assert np.array_equal(ys[v | 1], ys[1]), (name, dtype, v | 1, g)
            narrow = M.shape[1] <= K["CI16_MAX"]
            for g in STREAM_GROUPS:
                op.tune(STREAM, g)
                y8 = _twice(dev, ref, worst, (name, dtype, STREAM, g))
                for v in (STREAM | NT, STREAM | XCD, STREAM | PAGED, STREAM | NT | PAGED):
                    op.tune(v, g)
                    assert np.array_equal(_twice(dev, ref, worst, (name, dtype, v, g)), y8), (name, dtype, v, g)
                    if narrow and v & PAGED:
                        with gpu_ctx.options(paged16=0):
                            assert np.array_equal(dev.product(), y8), (name, dtype, v, g, "paged16=0")
    finally:
        op.close()
    worst.report()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_65536_and_65537_columns_give_the_same_bits(gpu_ctx, dtype):
    """The same entries with narrowed (65536 columns) and with 32-bit indices (65537 columns, x padded with
    one value that no entry reads)."""
    Ma, xa = SC.case("width_ci16")
    Mb, xb = SC.case("width_ci16_plus1")
    assert np.array_equal(xa, xb[:-1])
    ref = SC.reference("width_ci16", dtype)
    worst = _Worst(f"65536 vs 65537 columns {FT[dtype].__name__}")
    a = hgmres.SparseOperator.from_scipy(Ma, gpu_ctx, dtype=dtype)
    b = hgmres.SparseOperator.from_scipy(Mb, gpu_ctx, dtype=dtype)
    try:
        with _Dev(gpu_ctx, a, xa) as da, _Dev(gpu_ctx, b, xb) as db:
            for variants, groups in (((0, 1), ROW_GROUPS), ((STREAM, STREAM | PAGED), STREAM_GROUPS)):
                for v in variants:
                    for g in groups:
                        a.tune(v, g)
                        b.tune(v, g)
                        ya = _twice(da, ref, worst, ("65536", dtype, v, g))
                        assert np.array_equal(ya, _twice(db, ref, worst, ("65537", dtype, v, g))), (dtype, v, g)
    finally:
        a.close()
        b.close()
    worst.report()


# ---------------------------------------------------------------------------------------------
# bands
# ---------------------------------------------------------------------------------------------
BAND_LANES = (0, 8, 16, 32, 64)
BAND_VARIANTS = (0, 1, NT, STREAM, STREAM | PAGED)


def _band_sweep(ctx, M, x, ref, dtype, widths, worst, what):
    cols = M.shape[1]
    op = hgmres.SparseOperator.from_scipy(M, ctx, dtype=dtype)
    try:
        with _Dev(ctx, op, x) as dev:
            plain = {}
            op.set_bands(0, 0)
            for v in BAND_VARIANTS:
                op.tune(v, 0)
                plain[v] = _twice(dev, ref, worst, (what, dtype, "no bands", v))
            for W in widths:
                for g in BAND_LANES:
                    op.set_bands(W, g)
                    for v in BAND_VARIANTS:
                        op.tune(v, 0)
                        y = _twice(dev, ref, worst, (what, dtype, W, g, v))
                        if W >= cols:
                            assert np.array_equal(y, plain[v]), (what, dtype, W, g, v)
    finally:
        op.close()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["chunk_multiple_plus1", "width_ci16", "width_col_past16", "unsorted"])
def test_bands_of_every_width(gpu_ctx, name, dtype):
    """set_bands with cols - 1 (a last band of one column), cols // 5 + 1, cols and cols + 1 (no bands: the
    unbanded bits), band kernel lanes 0 (automatic), 8, 16, 32, 64, each followed by the band kernel
    (variants 0, 1, 2) and the banded streaming kernel (8, 8|16)."""
    M, x = SC.case(name)
    cols = M.shape[1]
    worst = _Worst(f"bands {name} {FT[dtype].__name__}")
    _band_sweep(gpu_ctx, M, x, SC.reference(name, dtype), dtype, (cols - 1, cols // 5 + 1, cols, cols + 1), worst, name)
    worst.report()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bands_of_one_column(gpu_ctx, dtype):
    """Case 2 restricted to its first 37 columns, in bands of one column: 37 bands, most (band, row)
    segments empty, none longer than one entry."""
    M = SC.restrict_columns(SC.case("pairs")[0], 37)
    x = SC.case("pairs")[1][:37]
    assert M.shape[1] == 37 and 0 < M.nnz and np.diff(M.indptr).max() <= 37 and np.any(np.diff(M.indptr) == 0)
    worst = _Worst(f"bands of one column {FT[dtype].__name__}")
    _band_sweep(gpu_ctx, M, x, SC.Reference(M, x, dtype), dtype, (1, 36, 37, 38), worst, "pairs[:, :37]")
    worst.report()


# ---------------------------------------------------------------------------------------------
# an x that is not 16-byte aligned
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_unaligned_x_gives_the_aligned_bits(gpu_ctx, dtype):
    """hgm_spmv with the x pointer advanced by one element (the paged gather needs 16-byte alignment and
    is dropped for that call): variants 1, 8|16 and banded 8|16 on case 1."""
    name = "chunk_multiple_plus1"
    M, x = SC.case(name)
    ref = SC.reference(name, dtype)
    worst = _Worst(f"unaligned x {FT[dtype].__name__}")
    op = hgmres.SparseOperator.from_scipy(M, gpu_ctx, dtype=dtype)
    try:
        with _Dev(gpu_ctx, op, x) as dev:
            for bands, v in ((0, 1), (0, STREAM | PAGED), (M.shape[1] // 5 + 1, STREAM | PAGED)):
                op.set_bands(bands, 0)
                for g in (STREAM_GROUPS if v & STREAM else ROW_GROUPS):
                    op.tune(v, g)
                    y = _twice(dev, ref, worst, (dtype, bands, v, g, "aligned"))
                    yu = _twice(dev, ref, worst, (dtype, bands, v, g, "unaligned"), unaligned=True)
                    assert np.array_equal(y, yu), (dtype, bands, v, g)
    finally:
        op.close()
    worst.report()


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_builders_against_numpy(gpu_ctx, name, dtype):
    """create_csr keeps the arrays as given; the transpose is the stable sort by column (scipy's
    csr -> csc conversion); its transpose is the row-sorted original; create_csc hands over the same
    entries.  Column counts 1, 2, 65536 and 65537 are the 1-, 16- and 17-bit radix sorts."""
    M, _ = SC.case(name)
    ops = []
    try:
        op = hgmres.SparseOperator.from_scipy(M, gpu_ctx, dtype=dtype)
        ops.append(op)
        assert op.shape == M.shape and op.nnz == M.nnz
        _same_csr(op.to_scipy(), M.indptr, M.indices, M.data, dtype, (name, "upload"))
        T = _transpose(gpu_ctx, op)
        ops.append(T)
        assert T.shape == M.shape[::-1] and T.nnz == M.nnz
        tp, ti, td = SC.stable_transpose(M)
        _same_csr(T.to_scipy(), tp, ti, td, dtype, (name, "transpose"))
        if M.has_canonical_format:                  # scipy's own transpose, where it is defined bit for bit
            St = M.T.tocsr()
            St.sort_indices()
            assert np.array_equal(St.indptr, tp) and np.array_equal(St.indices, ti) and np.array_equal(St.data, td)
        TT = _transpose(gpu_ctx, T)
        ops.append(TT)
        _same_csr(TT.to_scipy(), *SC.row_sorted(M), dtype, (name, "transpose of transpose"))
        Cc = hgmres.SparseOperator.from_csc(M, gpu_ctx, dtype=dtype)
        ops.append(Cc)
        assert Cc.shape == M.shape and Cc.nnz == M.nnz
        got = Cc.to_scipy()
        # (equal entries of one row and column may come in either order: compared as a multiset)
        for g, w in zip(SC.canonical_order(got.indptr, got.indices, got.data),
                        SC.canonical_order(M.indptr, M.indices, _rounded(M.data, dtype))):
            assert np.array_equal(g, w), (name, "from_csc")
        same_row = np.diff(np.repeat(np.arange(M.shape[0]), np.diff(got.indptr))) == 0
        assert np.all(np.diff(got.indices)[same_row] >= 0), (name, "from_csc: rows sorted by column")
    finally:
        for o in ops:
            o.close()


def _rows_of(M, lo, hi):
    p = M.indptr
    return (p[lo:hi + 1] - p[lo]).astype(np.int64), M.indices[p[lo]:p[hi]], M.data[p[lo]:p[hi]]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_slices(gpu_ctx, dtype):
    """row_slice over all rows, over no rows, inside and across runs of empty rows, over rows without
    entries, and of a slice: the rows of the parent, and under the row kernel the parent's product bits
    (scalar loads at any offset; paired loads where the slice starts at an even entry, which keeps the
    parity of every row start and with it the peeled heads and tails)."""
    name = "chunk_multiple_plus1"
    M, x = SC.case(name)
    rows = M.shape[0]
    run = np.flatnonzero((np.diff(M.indptr) == 0) & (M.indptr[:-1] == SCH))
    i0 = int(run[0])
    assert run.size >= 3 and np.all(np.diff(M.indptr)[-3:] == 0)
    windows = [(0, rows), (0, 0), (7, 7), (rows, rows), (i0 + 1, rows - 1), (i0, i0 + 3), (i0 + 1, i0 + 2), (3, rows - 2)]
    parent = hgmres.SparseOperator.from_scipy(M, gpu_ctx, dtype=dtype)
    ops = [parent]
    worst = _Worst(f"row slices {FT[dtype].__name__}")
    ref = SC.reference(name, dtype)
    try:
        with _Dev(gpu_ctx, parent, x) as dev:
            full = {}
            for v in (0, 1):
                for g in ROW_GROUPS:
                    parent.tune(v, g)
                    full[v, g] = _twice(dev, ref, worst, ("parent", dtype, v, g))

            def check(S, lo, hi, what):
                assert S.shape == (hi - lo, M.shape[1]) and S.nnz == M.indptr[hi] - M.indptr[lo], what
                _same_csr(S.to_scipy(), *_rows_of(M, lo, hi), dtype, what)
                if hi == lo:
                    return
                for v in (0, 1):
                    if v == 1 and M.indptr[lo] % 2:
                        continue
                    for g in ROW_GROUPS:
                        S.tune(v, g)
                        y = dev.product(S)
                        assert np.array_equal(y, dev.product(S)), what
                        assert np.array_equal(y, full[v, g][lo:hi]), (what, v, g)

            for lo, hi in windows:
                S = parent.row_slice(lo, hi)
                ops.append(S)
                check(S, lo, hi, ("slice", dtype, lo, hi))
            S2 = ops[-1].row_slice(1, 30)           # rows [4, 33) of the parent, through the empty run at SCH
            ops.append(S2)
            assert 4 < i0 and i0 + 3 < 33
            check(S2, 4, 33, ("slice of a slice", dtype))
            S3 = S2.row_slice(i0 - 4 + 1, i0 - 4 + 2)
            ops.append(S3)
            check(S3, i0 + 1, i0 + 2, ("slice of a slice, inside the empty run", dtype))
    finally:
        for o in ops:
            o.close()
    worst.report()


# ---------------------------------------------------------------------------------------------
# epilogues on the edges
# ---------------------------------------------------------------------------------------------
def _tuned_pair(ctx, config):
    A, _, _, _ = _solver_problem()
    Ao = hgmres.SparseOperator.from_scipy(A, ctx)
    Bo = _transpose(ctx, Ao)
    for o in (Ao, Bo):
        if config == "banded":
            o.set_bands(o.shape[1] // 5 + 1, 0)
        o.tune({"rows": 0, "paired": 1, "stream": STREAM | NT | PAGED, "banded": STREAM | NT | PAGED}[config], 0)
    return Ao, Bo


@gpu
@pytest.mark.parametrize("config", ["rows", "paired", "stream", "banded"])
@pytest.mark.parametrize("tag", sorted(SOLVERS))
def test_solver_epilogues_on_the_chunk_edges(gpu_ctx, tag, config):
    """hybrid_ab / hybrid_ba GMRES, 4 steps, on case 1 and its device transpose (empty rows in both):
    B (A v) + lambda v, v / h, the written-back q and the fused residual norm meet rows that no chunk
    owns entries of."""
    A, B, b, xt = _solver_problem()
    xr, er, rr, kr, Hr = _solver_oracle(tag)
    Ao, Bo = _tuned_pair(gpu_ctx, config)
    try:
        _same_csr(Bo.to_scipy(), B.indptr, B.indices, B.data, 0, "device transpose")
        x, e, r, k, H = SOLVERS[tag][0](Ao, Bo, b, xt, 0.0, STEPS, LAM, ctx=gpu_ctx, return_H=True)
    finally:
        Ao.close()
        Bo.close()
    assert k == kr == STEPS
    print(f"solver {tag} {config}: |dH| {np.max(np.abs(H - Hr)) / np.max(np.abs(Hr)):.2e} |dx| {rel(x, xr):.2e}")
    H_ok(H, Hr)
    assert rel(x, xr) < TOL
    hist_ok(r, rr, TOL)
    hist_ok(e, er, TOL)
