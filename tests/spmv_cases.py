"""Structure-edge matrices for the SpMV kernels and the operator builders (test_gpu_spmv_structure.py),
with their wide-precision reference products.  Plain helper module: the CPU tests assert that every case
has the property it is named for, the GPU tests run the kernels on it.

The sizes follow the code: SCH (entries per streaming chunk), the page limits of the paged gather, the
unroll of the paired-load row loop, the lane ladders and the 16-bit index limit are read from csrc/ by
regular expression (constants()), so a constant that moves there moves the cases with it."""
import functools
import os
import re
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-gmres_amd", "csrc")


# ---------------------------------------------------------------------------------------------
# constants of csrc/
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """SCH, PG_BYTES, PG_MAX64, PG_MAX32, PG_ROUNDS32, SPMV_U, CI16_MAX (the largest column count whose
    indices build_ci16 narrows), ROW_GROUPS, BAND_GROUPS, STREAM_GROUPS as csrc/ states them."""
    src = {}
    for f in ("internal.h", "spmv.hip", "ops.hip"):
        with open(os.path.join(CSRC, f)) as fh:
            src[f] = fh.read()
    v = {}

    def define(name, text):
        mt = re.search(r"#define[ \t]+%s[ \t]+([^\n]+)" % name, text)
        assert mt, name
        expr = mt.group(1).split("//")[0].strip()
        assert re.fullmatch(r"[\w\s*+/()-]+", expr), (name, expr)
        return int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(v)))

    v["HGM_SCH"] = define("HGM_SCH", src["internal.h"])
    assert re.search(r"constexpr\s+int\s+SCH\s*=\s*HGM_SCH\s*;", src["internal.h"])
    v["SCH"] = v["HGM_SCH"]
    mt = re.search(r"constexpr\s+int\s+PG_BYTES\s*=\s*(\d+)\s*;", src["internal.h"])
    assert mt, "PG_BYTES"
    v["PG_BYTES"] = int(mt.group(1))
    v["PG_MAX64"] = define("HGM_PG_MAX64", src["internal.h"])
    v["PG_MAX32"] = define("HGM_PG_MAX32", src["internal.h"])
    v["PG_ROUNDS32"] = define("HGM_PG_ROUNDS32", src["internal.h"])
    v["SPMV_U"] = define("HGM_SPMV_U", src["spmv.hip"])
    body = re.search(r"static void build_ci16\([^)]*\)\s*\{(.*?)\n\}", src["ops.hip"], re.S)
    assert body, "build_ci16"
    mt = re.search(r"M->cols\s*>\s*(\d+)", body.group(1))
    assert mt, "build_ci16 limit"
    v["CI16_MAX"] = int(mt.group(1))
    for key, name in (("ROW_GROUPS", "RowGroups"), ("BAND_GROUPS", "BandGroups"), ("STREAM_GROUPS", "StreamGroups")):
        mt = re.search(r"using\s+%s\s*=\s*Ints<([\d,\s]+)>\s*;" % name, src["internal.h"])
        assert mt, name
        v[key] = tuple(int(t) for t in mt.group(1).split(","))
    return v


# ---------------------------------------------------------------------------------------------
# construction helpers
# ---------------------------------------------------------------------------------------------
def _csr(rows, n, rng):
    """CSR (not canonicalised by scipy: the arrays are handed over as built) from a list of per-row
    column arrays, standard normal values"""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = (np.concatenate(rows) if rows else np.empty(0)).astype(np.int32)
    data = rng.standard_normal(indices.size)
    return sp.csr_matrix((data, indices, indptr), shape=(len(rows), n))


def _from_lengths(lengths, n, rng):
    return _csr([np.sort(rng.choice(n, size=int(L), replace=False)) for L in lengths], n, rng)


# ---------------------------------------------------------------------------------------------
# case 1: streaming chunk edges
# ---------------------------------------------------------------------------------------------
N_CHUNK = 12001


def chunk_edge_lengths(S, plus_one, rng):
    """Row lengths whose running entry count puts row ends, row starts, runs of empty rows and the end
    of the matrix on multiples of the chunk size S (the comments name the property each row is for)."""
    L = []

    def to(target):
        assert target > sum(L)
        L.append(target - sum(L))

    L += [0, 0]                         # leading empty rows
    L += [5, 100]
    to(S)                               # a row ending exactly at S
    L += [0, 0, 0]                      # empty rows whose pointer equals S
    to(2 * S)                           # a row of exactly S entries occupying chunk [S, 2S)
    L += [1]                            # a single-entry row right after the boundary 2S
    to(3 * S - 150)                     # starts and ends mid-chunk, inside one chunk
    to(5 * S + 300)                     # starts mid-chunk, covers whole chunks, ends mid-chunk: > 2S entries
    to(6 * S)                           # starts mid-chunk, ends exactly on a boundary
    L += [1]
    L += [int(v) for v in rng.integers(0, 80, 20)]
    to(7 * S - 1)
    L += [1, 1]                         # single-entry rows on both sides of the boundary 7S
    L += [int(v) for v in rng.integers(0, 80, 10)]
    to(8 * S)                           # the total is a multiple of S ...
    if plus_one:
        L += [1]                        # ... plus one entry: a last chunk of one entry
    L += [0, 0, 0]                      # trailing empty rows
    return L


def small_lengths(total):
    """a matrix of `total` entries in one (partial or exactly full) chunk, with empty rows around"""
    return [0, 0, 33, 0, 1, total - 33 - 1 - 1200 - 1, 1200, 1, 0, 0]


# ---------------------------------------------------------------------------------------------
# case 2: row bounds of the paired loads
# ---------------------------------------------------------------------------------------------
def pair_lengths(G):
    """0, 1, 2, 3 and the steps of seg_partial<VEC>'s loops (2G, 4G and U*2G = 8G entries at U = 4), +-1"""
    U = constants()["SPMV_U"]
    return [0, 1, 2, 3, 2 * G - 1, 2 * G, 2 * G + 1, 4 * G - 1, 4 * G + 1, 2 * U * G - 1, 2 * U * G,
            2 * U * G + 1, 4 * U * G + 1]


def pair_plan():
    """[(G, length, parity)] in row order, a one-entry row (G = 0) wherever the parity has to flip"""
    plan, pos = [], 0
    for G in constants()["ROW_GROUPS"]:
        for L in pair_lengths(G):
            for parity in (0, 1):
                if pos % 2 != parity:
                    plan.append((0, 1, pos % 2))
                    pos += 1
                plan.append((G, L, parity))
                pos += L
    return plan


# The longest row (16 G + 1 = 1025 entries at 64 lanes) needs that many distinct columns: 1031, not ~700.
N_PAIR = 1031


# ---------------------------------------------------------------------------------------------
# case 3: index width
# ---------------------------------------------------------------------------------------------
def _index_width_rows(rng, top):
    """48 rows of 200-380 sorted columns, each with 0, top // 2, top // 2 + 1 and top (top = 65535: the
    16-bit limit; columns top - 1 and above top are left free)"""
    rows = []
    pool = np.setdiff1d(np.arange(1, top - 1), [top // 2, top // 2 + 1])
    for L in rng.integers(200, 381, 48):
        mid = rng.choice(pool, size=int(L) - 4, replace=False)
        rows.append(np.sort(np.concatenate([mid, [0, top // 2, top // 2 + 1, top]])))
    return rows


# ---------------------------------------------------------------------------------------------
# case 4: page limits
# ---------------------------------------------------------------------------------------------
N_PAGE = 20011          # 11 mod 16 and 11 mod 32: the last page of x is partial in both types


def _paged_chunks(page_counts, E, n, S, rng):
    """Full chunks (four rows of S / 4 entries, an empty row after each chunk) touching exactly
    page_counts[k] distinct E-element pages of x, then one full chunk of 100 pages that holds the last
    column n - 1 (in the last, partial page), then a 100-entry row (a final partial chunk)."""
    assert S % 4 == 0 and n % E
    q = S // 4
    rows = []
    for k, P in enumerate(list(page_counts) + [100]):
        last = k == len(page_counts)
        assert P <= q and P * E >= q
        pages = rng.choice(n // E, size=P - 1 if last else P, replace=False)
        if last:
            pages = np.concatenate([pages, [n // E]])
        allowed = (pages[:, None] * E + np.arange(E)[None, :]).ravel()
        allowed = allowed[allowed < n]
        one_each = pages * E + rng.integers(0, E, pages.size)
        if last:
            one_each[-1] = n - 1
        rest = rng.choice(np.setdiff1d(allowed, one_each), size=q - one_each.size, replace=False)
        rows.append(np.sort(np.concatenate([one_each, rest])))
        for _ in range(3):
            rows.append(np.sort(rng.choice(allowed, size=q, replace=False)))
        rows.append(np.empty(0, int))
    rows.append(np.sort(rng.choice(n, size=100, replace=False)))
    return _csr(rows, n, rng)


def chunk_page_counts(M, E, S):
    """distinct E-element pages of x touched by the entries [k S, (k + 1) S) of the CSR stream, full chunks"""
    return [int(np.unique(M.indices[k * S:(k + 1) * S] // E).size) for k in range(M.nnz // S)]


# ---------------------------------------------------------------------------------------------
# case 6: unsorted and duplicate columns
# ---------------------------------------------------------------------------------------------
def _unsorted_duplicates(rng):
    n, rows = 9000, []
    for r, L in enumerate(rng.integers(150, 351, 40)):
        cols = rng.choice(n, size=int(L), replace=False)
        if r % 5 == 1:                  # one column two times, another three times
            cols[3] = cols[11]
            cols[20] = cols[40] = cols[7]
        rows.append(rng.permutation(cols))
    return _csr(rows, n, rng)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
CASE_NAMES = ("chunk_multiple", "chunk_multiple_plus1", "chunk_minus1", "chunk_exact",
              "pairs",
              "width_ci16", "width_ci16_plus1", "width_col_past16", "width_ci16_minus1",
              "pages64", "pages32",
              "one_row", "one_col", "two_cols", "one_by_one", "last_row_only", "no_entries",
              "unsorted")


def pages64_counts():
    return [constants()["PG_MAX64"], constants()["PG_MAX64"] + 1]


def pages32_counts():
    p = constants()["PG_MAX32"]
    r = constants()["PG_ROUNDS32"]
    return [p, p + 1, r * p, r * p + 1]


@functools.lru_cache(maxsize=None)
def case(name):
    """(M, x): the CSR matrix (arrays as built, never canonicalised) and the fp64 vector of case `name`"""
    c = constants()
    S, top = c["SCH"], c["CI16_MAX"] - 1
    rng = np.random.default_rng(2026 + CASE_NAMES.index(name))
    if name == "chunk_multiple":
        M = _from_lengths(chunk_edge_lengths(S, False, rng), N_CHUNK, rng)
    elif name == "chunk_multiple_plus1":
        M = _from_lengths(chunk_edge_lengths(S, True, rng), N_CHUNK, rng)
    elif name == "chunk_minus1":
        M = _from_lengths(small_lengths(S - 1), N_CHUNK, rng)
    elif name == "chunk_exact":
        M = _from_lengths(small_lengths(S), N_CHUNK, rng)
    elif name == "pairs":
        M = _from_lengths([L for _, L, _ in pair_plan()], N_PAIR, rng)
    elif name.startswith("width_"):
        rng = np.random.default_rng(2026)           # the four operators share rows and values
        rows = _index_width_rows(rng, top)
        cols = {"width_ci16": top + 1, "width_ci16_plus1": top + 2, "width_col_past16": top + 2,
                "width_ci16_minus1": top}[name]
        M = _csr(rows, cols, rng)
        if name == "width_col_past16":              # one entry per row moved to column 65536
            for r in range(M.shape[0]):
                lo, hi = M.indptr[r], M.indptr[r + 1]
                j = lo + 7 + r % 5
                v = M.data[j]
                M.indices[j:hi - 1] = M.indices[j + 1:hi].copy()
                M.data[j:hi - 1] = M.data[j + 1:hi].copy()
                M.indices[hi - 1], M.data[hi - 1] = top + 1, v
        if name == "width_ci16_minus1":             # the largest column is 65534
            M.indices[M.indices == top] = top - 1
    elif name == "pages64":
        M = _paged_chunks(pages64_counts(), c["PG_BYTES"] // 8, N_PAGE, S, rng)
    elif name == "pages32":
        M = _paged_chunks(pages32_counts(), c["PG_BYTES"] // 4, N_PAGE, S, rng)
    elif name == "one_row":
        M = _from_lengths([10000], 10000, rng)
    elif name == "one_col":
        M = _from_lengths([int(v) for v in rng.integers(0, 2, 300)], 1, rng)
    elif name == "two_cols":                        # (with one_col: the 1-bit radix sort of the transpose)
        M = _from_lengths([2, 0, 1, 1, 2, 0, 0, 1, 2], 2, rng)
    elif name == "one_by_one":
        M = _from_lengths([1], 1, rng)
    elif name == "last_row_only":
        M = _from_lengths([0] * 199 + [37], 50, rng)
    elif name == "no_entries":
        M = _from_lengths([0] * 4, 3, rng)
    elif name == "unsorted":
        M = _unsorted_duplicates(rng)
    else:
        raise KeyError(name)
    x = np.random.default_rng(7 + CASE_NAMES.index(name)).standard_normal(M.shape[1])
    if name.startswith("width_"):                   # one x: the 65537-column operators read one value more
        x = np.random.default_rng(7).standard_normal(top + 2)[: M.shape[1]]
    return M, x


def restrict_columns(M, ncols):
    """the entries of M in columns < ncols, as a rows x ncols matrix (row order kept)"""
    keep = M.indices < ncols
    rowidx = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))[keep]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rowidx, minlength=M.shape[0]))]).astype(np.int64)
    return sp.csr_matrix((M.data[keep], M.indices[keep], indptr), shape=(M.shape[0], ncols))


# ---------------------------------------------------------------------------------------------
# reference product and bounds
# ---------------------------------------------------------------------------------------------
WIDE_OK = np.finfo(np.longdouble).eps < 2.0 ** -53
UNIT = {0: 2.0 ** -53, 1: 2.0 ** -24}               # unit roundoff of the operator's type (0 fp64, 1 fp32)


class Reference:
    """Row sums of M x over the CSR arrays in a wide type (np.longdouble where it is wider than
    fp64, else exact fractions), from inputs rounded to the operator's type first.

    L[i]: stored entries of row i; s[i] = (|M| |x|)_i; slack[i]: the reference's own rounding error."""

    def __init__(self, M, x, dtype, wide=None):
        self.wide = WIDE_OK if wide is None else wide
        data, xv = M.data, np.asarray(x, dtype=np.float64)
        if dtype == 1:
            data, xv = data.astype(np.float32), xv.astype(np.float32)
        self.dtype = dtype
        self.L = np.diff(M.indptr).astype(np.int64)
        rows = M.shape[0]
        if self.wide:
            p = data.astype(np.longdouble) * xv.astype(np.longdouble)[M.indices]
            self.ref = np.zeros(rows, dtype=np.longdouble)
            s = np.zeros(rows, dtype=np.longdouble)
            for i in range(rows):
                lo, hi = M.indptr[i], M.indptr[i + 1]
                self.ref[i] = p[lo:hi].sum()
                s[i] = np.abs(p[lo:hi]).sum()
            self.s = s.astype(np.float64)
            self.slack = (self.L + 1) * float(np.finfo(np.longdouble).eps) * self.s
        else:
            self.ref, s = [], []
            for i in range(rows):
                lo, hi = M.indptr[i], M.indptr[i + 1]
                t = [Fraction(float(data[j])) * Fraction(float(xv[M.indices[j]])) for j in range(lo, hi)]
                self.ref.append(sum(t, Fraction(0)))
                s.append(float(sum((abs(v) for v in t), Fraction(0))))
            self.s = np.array(s, dtype=np.float64)
            self.slack = np.zeros(rows)

    def errors(self, y):
        y = np.asarray(y, dtype=np.float64)
        if self.wide:
            return np.abs(y.astype(np.longdouble) - self.ref).astype(np.float64)
        return np.array([float(abs(Fraction(float(v)) - r)) for v, r in zip(y, self.ref)])

    def derived_bound(self):
        """gamma(L + 1) s, gamma(k) = k u / (1 - k u): a length-L dot product in any summation order"""
        k = (self.L + 1) * UNIT[self.dtype]
        return k / (1.0 - k) * self.s + self.slack

    def check(self, y, what=""):
        """Asserts the bounds of the issue on one product; returns the largest ratios
        (to the derived bound, to the project bound 1e-14 (s + 1e-300); the latter fp64 only, else nan)."""
        y = np.asarray(y, dtype=np.float64)
        assert y.shape == self.s.shape, (what, y.shape)
        assert np.all(np.isfinite(y)), (what, "row not written", np.flatnonzero(~np.isfinite(y))[:8])
        empty = self.L == 0
        assert np.all(y[empty] == 0.0), (what, "empty row not 0", np.flatnonzero(empty & (y != 0))[:8])
        err = self.errors(y)
        one = self.L == 1                            # a single product: one rounding
        lim1 = UNIT[self.dtype] * self.s + self.slack
        assert np.all(err[one] <= lim1[one]), (what, "one-entry row", np.flatnonzero(one & (err > lim1))[:8])
        full = ~empty
        rd = float(np.max(err[full] / self.derived_bound()[full])) if full.any() else 0.0
        assert rd <= 1.0, (what, "derived bound", rd, int(np.argmax(err / np.maximum(self.derived_bound(), 1e-300))))
        rp = float("nan")
        if self.dtype == 0:
            rp = float(np.max(err / (1e-14 * (self.s + 1e-300))))
            assert rp <= 1.0, (what, "1e-14 bound", rp)
        return rd, rp


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    M, x = case(name)
    return Reference(M, x, dtype)


def summed_dense_product(M, x, dtype):
    """(D x, |D| |x|) in np.longdouble, D the dense matrix of M with duplicate entries summed in
    np.longdouble (small matrices only)"""
    data, xv = M.data, np.asarray(x, dtype=np.float64)
    if dtype == 1:
        data, xv = data.astype(np.float32), xv.astype(np.float32)
    D = np.zeros(M.shape, dtype=np.longdouble)
    rowidx = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    np.add.at(D, (rowidx, M.indices), data.astype(np.longdouble))
    xw = xv.astype(np.longdouble)
    return D @ xw, np.abs(D) @ np.abs(xw)


# ---------------------------------------------------------------------------------------------
# builder references (numpy only, bit for bit)
# ---------------------------------------------------------------------------------------------
def stable_transpose(M):
    """(indptr, indices, data) of M' with the entries of every output row in CSR stream order of M: the
    stable order of the device transpose, and scipy's csr -> csc conversion"""
    rowidx = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.argsort(M.indices, kind="stable")
    indptr = np.concatenate([[0], np.cumsum(np.bincount(M.indices, minlength=M.shape[1]))]).astype(np.int64)
    return indptr, rowidx[order].astype(np.int32), M.data[order]


def row_sorted(M):
    """(indptr, indices, data) of M with every row stably sorted by column (duplicates keep their order)"""
    rowidx = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.lexsort((np.arange(M.nnz), M.indices, rowidx))
    return M.indptr.astype(np.int64), M.indices[order].astype(np.int32), M.data[order]


def canonical_order(indptr, indices, data):
    """entries sorted by (row, column, value): equal for two CSR forms of one multiset of entries"""
    rowidx = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    order = np.lexsort((data, indices, rowidx))
    return np.asarray(indptr, dtype=np.int64), np.asarray(indices)[order], np.asarray(data)[order]
