"""Structure-edge operators for the one-pass A*(B*q) row-wave plan and kernel (test_gpu_fused_structure.py):
case builders, a CPU twin of the plan rules of csrc/fused.hip (fused_plan_build_rw, fused_plan_dev_finish,
fused_plan_vstream, fused_ab_plan) and the references of the two products.  Plain helper module.

An operator is a scipy CSR over reference-order pixel columns of a tiled N x N grid (what
SparseOperator.from_scipy_tiled takes); the plan sees its transpose B in the stored pixel order, rows =
pixels, the entries of a row in ray order (BView).  The cases are built in that stored order, row by row, and
the CPU tests prove with the twin, from the CSR alone, that each case has the property it is named for.  The
twin is a checker: it restates the rules once, in numpy, and nothing in the library reads it.

The sizes follow the code: the constants are read from csrc/ by regular expression (constants())."""
import functools
import os
import re

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid-gmres_amd", "csrc")
TILE = 4
WAVES = 4


# ---------------------------------------------------------------------------------------------
# constants of csrc/
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def constants():
    """RW_ROW_MAX, RW_SLOTS_MAX, SHAPES (the production four-wave LDS shapes), VS_CODES, CHUNK (entries of a
    row pair's chunk), RUN_CAP (runs per wave), PLAN_DEV_MAX_M, LIDX_PAD, REGION (the default region side)."""
    with open(os.path.join(CSRC, "fused.hip")) as fh:
        src = fh.read()
    with open(os.path.join(CSRC, "internal.h")) as fh:
        hdr = fh.read()

    def one(pattern, text=src, what=None):
        mt = re.search(pattern, text)
        assert mt, what or pattern
        return mt

    v = {}
    v["RW_ROW_MAX"] = int(one(r"constexpr\s+int\s+RW_ROW_MAX\s*=\s*(\d+)\s*;").group(1))
    v["RW_SLOTS_MAX"] = int(one(r"constexpr\s+int\s+RW_SLOTS_MAX\s*=\s*(\d+)\s*;").group(1))
    shapes = one(r"#else\s*\n#define\s+HGM_RW_SHAPES\(X\)([^\n]*)\n#endif").group(1)
    pairs = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", shapes)]
    assert pairs and all(w == WAVES for w, _ in pairs), pairs
    v["SHAPES"] = tuple(sorted(s for _, s in pairs))
    v["VS_CODES"] = int(one(r"constexpr\s+int\s+VS_CODES\s*=\s*(\d+)\s*;").group(1))
    chunk = int(one(r"\(rp\[s \+ 2\] - rp\[s\]\) \+ \(rp\[s\] & 1\) <= (\d+)").group(1))
    assert int(one(r"maxlen \+ 1 <= (\d+)").group(1)) == chunk
    v["CHUNK"] = chunk
    cap = int(one(r"if \(out\.size\(\) > (\d+)\) over = true").group(1))
    assert int(one(r"HGM_REQUIRE\(wr\[i\]\.size\(\) <= (\d+)").group(1)) == cap
    v["RUN_CAP"] = cap
    mt = one(r"constexpr\s+int64_t\s+PLAN_DEV_MAX_M\s*=\s*int64_t\((\d+)\)\s*\*\s*(\d+)\s*\*\s*(\d+)\s*;")
    v["PLAN_DEV_MAX_M"] = int(mt.group(1)) * int(mt.group(2)) * int(mt.group(3))
    v["LIDX_PAD"] = int(one(r"hipMalloc\(&P->lidx, sizeof\(uint16_t\) \* \(nnz \+ (\d+)\)\)").group(1))
    v["REGION"] = int(one(r"int\s+fused_wregion\s*=\s*(\d+)\s*;", hdr).group(1))
    return v


# ---------------------------------------------------------------------------------------------
# the stored order and B's view of an operator
# ---------------------------------------------------------------------------------------------
def stored_pixel_index(N, tile=TILE):
    from hgmres.core import stored_pixel_index as spi
    return spi(N, tile, 0)


class BView:
    """B = A' in the stored pixel order: rp, ci (rays, ascending inside a row), val.  `N`: the grid; rows < N * N: a shard of whole tile columns from `lo`."""

    def __init__(self, N, m, rp, ci, val, lo=0):
        self.N, self.m, self.rp, self.ci, self.val, self.lo = N, m, rp, ci, val, lo
        self.rows = rp.size - 1
        self.len = np.diff(rp)
        self.nnz = int(rp[-1])
        self.rowidx = np.repeat(np.arange(self.rows), self.len)

    @classmethod
    def of(cls, S, N):
        """from the scipy CSR S (m x N^2, reference-order columns, explicit zeros kept)"""
        S = sp.csr_matrix(S)
        pos = stored_pixel_index(N)
        rays = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
        spix = pos[S.indices]
        order = np.lexsort((rays, spix))
        rp = np.concatenate([[0], np.cumsum(np.bincount(spix, minlength=N * N))]).astype(np.int64)
        return cls(N, S.shape[0], rp, rays[order].astype(np.int64), S.data[order].copy())

    def shard(self, lo, hi):
        a, b = self.rp[lo], self.rp[hi]
        return BView(self.N, self.m, self.rp[lo:hi + 1] - a, self.ci[a:b], self.val[a:b], lo=self.lo + lo)

    def with_values(self, val):
        return BView(self.N, self.m, self.rp, self.ci, val, self.lo)


# ---------------------------------------------------------------------------------------------
# the twin of the plan rules
# ---------------------------------------------------------------------------------------------
def row_regions(N, R, rows=None, tile=TILE):
    """(region of every stored row, number of regions): fused.hip row_regions, the whole grid from
    stored_pixel_index, a shard of whole tile columns from its own first column"""
    rows = N * N if rows is None else rows
    nbr = -(-N // R)
    if rows == N * N:
        p = np.arange(N * N)
        reg = np.empty(N * N, dtype=np.int64)
        reg[stored_pixel_index(N, tile)] = (p // N // R) * nbr + (p % N) // R
        return reg, nbr * nbr
    assert rows % (tile * N) == 0
    s = np.arange(rows)
    tl, w = s // (tile * tile), s % (tile * tile)
    tpc = N // tile
    r, c = (tl % tpc) * tile + w % tile, (tl // tpc) * tile + w // tile
    return (c // R) * nbr + r // R, nbr * -(-(rows // N) // R)


def region_rows(reg, nreg):
    """the stored rows of every region, in stored order"""
    return [np.flatnonzero(reg == g) for g in range(nreg)]


def _append(runs, s):
    if runs and runs[-1][0] + runs[-1][1] == s:
        runs[-1][1] += 1
    else:
        runs.append([int(s), 1])


def wave_shares(rows_g, rp, W=WAVES):
    """the W contiguous shares (by entries) of a region's rows, each as runs [first row, rows]"""
    tot = int(sum(rp[s + 1] - rp[s] for s in rows_g))
    out = [[] for _ in range(W)]
    w, done = 0, 0
    for s in rows_g:
        while w < W - 1 and done * W >= tot * (w + 1):
            w += 1
        _append(out[w], s)
        done += int(rp[s + 1] - rp[s])
    return out


def pair_fits(rp, s, chunk):
    return (rp[s + 2] - rp[s]) + (rp[s] & 1) <= chunk


def pair_cuts(runs, rp, chunk):
    """row-pair mode 4: rows 2i, 2i + 1 of a run are a unit; a unit that does not fit the chunk ends the run
    after its first row"""
    out = []
    for x, y in runs:
        s0 = s = x
        end = x + y
        while s < end:
            if s + 1 < end and not pair_fits(rp, s, chunk):
                out.append([s0, s + 1 - s0])
                s0 = s = s + 1
            else:
                s += 2
        if s0 < end:
            out.append([s0, end - s0])
    return out


def _plan_at(bv, R, rowpair, es):
    K = constants()
    maxlen = int(bv.len.max()) if bv.rows else 0
    p = dict(region=R, maxlen=maxlen, refused=None, rowpair=False)
    if maxlen > K["RW_ROW_MAX"]:
        p["refused"] = "row"
        return p
    reg, nreg = row_regions(bv.N, R, bv.rows)
    rows = region_rows(reg, nreg)
    wr = [share for g in range(nreg) for share in wave_shares(rows[g], bv.rp)]
    pairs_on = bool(rowpair) and maxlen + 1 <= K["CHUNK"]
    if pairs_on:
        cut = [pair_cuts(r, bv.rp, K["CHUNK"]) for r in wr]
        if max(len(r) for r in cut) > K["RUN_CAP"]:
            pairs_on = False
        else:
            wr = cut
    p.update(rowpair=pairs_on, wave_runs=wr, nruns=sum(len(r) for r in wr), nreg=nreg, reg=reg,
             runs_per_wave=[len(r) for r in wr])
    if max(len(r) for r in wr) > K["RUN_CAP"]:
        p["refused"] = "runs"
        return p
    rays = [np.unique(bv.ci[np.isin(bv.rowidx, rows[g])]) for g in range(nreg)]
    p["rays"] = rays
    p["count"] = [int(r.size) for r in rays]
    p["worst"] = max(p["count"])
    p["nslot"] = sum(p["count"])
    fit = [s for s in K["SHAPES"] if p["worst"] <= s - 64]
    if not fit:
        p["refused"] = "lds"
        return p
    p["slots"] = fit[0]
    return p


def value_dictionary(val, room):
    """fused_plan_vstream's codes: the most frequent bit patterns (seen twice or more; finite, normal, not
    zero; ties by bit pattern), at most `room`"""
    bits = np.ascontiguousarray(val, dtype=np.float64).view(np.uint64)
    u, c = np.unique(bits, return_counts=True)
    ex = (u >> np.uint64(52)) & np.uint64(0x7FF)
    ok = (c >= 2) & (ex != 0) & (ex != 0x7FF)
    cand = sorted(zip((-c[ok]).tolist(), u[ok].tolist()))
    return np.array(sorted(b for _, b in cand[:max(room, 0)]), dtype=np.uint64)


def twin_plan(bv, rowpair=4, vstream=0, es=8):
    """The plan fused_ab_plan arrives at: region (after the halving retry), refused (None, "row", "runs",
    "lds"), rowpair, wave_runs, nruns, worst, slots, nslot, compact, codes (count), code_bits."""
    K = constants()
    R = K["REGION"]
    while True:
        p = _plan_at(bv, R, rowpair, es)
        if p["refused"] == "lds" and R // 2 >= 16 and R % 2 == 0:
            R //= 2
            continue
        break
    p["tried"] = K["REGION"] // R
    p["compact"], p["codes"], p["code_bits"] = False, None, None
    if p["refused"]:
        return p
    if (vstream and es == 8 and p["rowpair"] and rowpair == 4 and p["slots"] <= 2048 and p["worst"] <= p["slots"] - 65
            and bv.nnz > 0 and not np.any(np.isnan(bv.val))):
        room = min(K["VS_CODES"], p["slots"] - 65 - p["worst"])
        d = value_dictionary(bv.val, room) if vstream != 2 else np.empty(0, dtype=np.uint64)
        coded = np.isin(np.ascontiguousarray(bv.val).view(np.uint64), d)
        nunit = sum((y + 1) // 2 for r in p["wave_runs"] for _, y in r)
        if vstream == 1:
            # (the byte rule of fused_plan_vstream: value pairs per unit from the unit layout)
            npairs = sum(u["pairs"] for u in units(bv, p, coded))
            worth = 16.0 * npairs + 264.0 * nunit <= (1.0 - 0.08) * (10.0 * bv.nnz + 8.0 * bv.rows)
            if d.size == 0 or not worth:
                return p
        p["compact"], p["codes"], p["code_bits"], p["coded"] = True, int(d.size), d, coded
    return p


def units(bv, plan, coded=None):
    """The units of a plan in plan order: dict(row, single, lenA, lenB, parity = rp[row] & 1, span, wave,
    and with `coded` (a mask over B's entries): codedA, codedB, c0h, pairs)."""
    out = []
    for w, runs in enumerate(plan["wave_runs"]):
        for x, y in runs:
            for k in range(0, y, 2 if plan["rowpair"] else 1):
                s = x + k
                single = (not plan["rowpair"]) or k + 1 == y
                a, b = int(bv.len[s]), (0 if single else int(bv.len[s + 1]))
                u = dict(row=s, single=single, lenA=a, lenB=b, parity=int(bv.rp[s] & 1), wave=w,
                         span=a + b + int(bv.rp[s] & 1))
                if coded is not None:
                    e = bv.rp[s]
                    cA, cB = int(coded[e:e + a].sum()), int(coded[e + a:e + a + b].sum())
                    nE = a + b - cA - cB
                    u.update(codedA=cA, codedB=cB, c0h=cA // 2, pairs=((cA & 1) + nE + 1) // 2 if nE else 0)
                out.append(u)
    return out


# ---------------------------------------------------------------------------------------------
# case construction: rows of B in the stored order
# ---------------------------------------------------------------------------------------------
ZERO_P, ZERO_M, SUBNORMAL = -1, -2, -3          # value ids of the special stored values
SPECIAL = {ZERO_P: 0.0, ZERO_M: -0.0, SUBNORMAL: 2.0 ** -1060}
KTAB = np.array([k * s for k in range(1, 21) for s in (1, -1)], dtype=np.int64)    # exact values KTAB / 16


class Case:
    """rows[s] = (rays, value ids) of stored pixel row s; m rays; an N x N grid in 4 x 4 tiles.
    value id v >= 0: real inputs take the v-th of a table of standard normal draws (so equal ids are equal
    bit patterns), exact inputs KTAB[v mod nk] / 16; v < 0: SPECIAL, in both."""

    def __init__(self, name, N, m, rows, note=""):
        self.name, self.N, self.m, self.note = name, N, m, note
        n = N * N
        inv = np.empty(n, dtype=np.int64)
        inv[stored_pixel_index(N)] = np.arange(n)
        r, c, v = [], [], []
        for s in sorted(rows):
            rays, ids = rows[s]
            rays = np.asarray(rays, dtype=np.int64)
            assert rays.size == 0 or (np.all(np.diff(rays) > 0) and 0 <= rays[0] and rays[-1] < m), (name, s)
            r.append(rays)
            c.append(np.full(rays.size, inv[s]))
            v.append(np.broadcast_to(np.asarray(ids, dtype=np.int64), rays.shape))
        r, c, v = (np.concatenate(a) if a else np.empty(0, np.int64) for a in (r, c, v))
        order = np.lexsort((c, r))
        self.ray, self.col, self.vid = r[order], c[order], v[order]
        self.indptr = np.concatenate([[0], np.cumsum(np.bincount(self.ray, minlength=m))]).astype(np.int64)

    def values(self, mode, dtype=0):
        """mode "real" or "exact"; dtype 1: rounded to fp32 (the exact values are fp32 numbers already)"""
        vid = self.vid
        if mode == "real":
            table = np.random.default_rng(4242).standard_normal(int(max(vid.max(initial=0), 0)) + 1)
            val = table[np.maximum(vid, 0)]
        else:
            nk = 8 if dtype == 1 else KTAB.size
            val = KTAB[np.maximum(vid, 0) % nk] / 16.0
        for k, x in SPECIAL.items():
            val = np.where(vid == k, x, val)
        return val.astype(np.float32).astype(np.float64) if dtype == 1 else val

    def matrix(self, mode="real", dtype=0):
        """the scipy CSR (m x N^2, reference-order columns; arrays as built, explicit zeros kept)"""
        return sp.csr_matrix((self.values(mode, dtype), self.col.astype(np.int32), self.indptr), shape=(self.m, self.N ** 2))

    def bview(self, mode="real", dtype=0):
        return BView.of(self.matrix(mode, dtype), self.N)


class _Seq:
    """Row lengths for consecutive rows of one run that starts at CSR entry rp0, with the unit structure of
    row-pair mode 4 tracked as the plan will form it (unit() places a pair at an even offset of its run with
    the wanted parity of its first entry)."""

    def __init__(self, chunk, rp0=0):
        self.chunk, self.rp, self.off, self.lens, self.first = chunk, rp0, 0, [], None

    def row(self, L):
        if self.off % 2 == 1 and self.first[0] + L + self.first[1] <= self.chunk:
            self.off += 1
        else:                                       # a unit's first row (after a cut: of a new run)
            self.first, self.off = (L, self.rp & 1), 1
        self.lens.append(L)
        self.rp += L

    def unit(self, a, b, parity):
        while self.off % 2:
            self.row(1)
        if (self.rp & 1) != parity:
            self.row(1)
            self.row(2)
        self.row(a)
        if b is not None:
            self.row(b)


def _pick(rng, pool, L):
    return np.sort(rng.choice(pool, size=int(L), replace=False))


def _ids(rng, L, kind):
    """value ids of L entries: "few" (16 values), "skew" (40 values, geometric), "distinct" (set by caller)"""
    if kind == "few":
        return rng.integers(0, 16, L)
    return np.minimum(rng.geometric(0.12, L) - 1, 39)


def _background(rng, rows, stored, pool, lo, hi, kind="skew"):
    for s in stored:
        if s not in rows:
            L = int(rng.integers(lo, hi + 1))
            rows[int(s)] = (_pick(rng, pool, L), _ids(rng, L, kind))


def _regions(N):
    reg, nreg = row_regions(N, constants()["REGION"])
    return region_rows(reg, nreg)


# --- A: rays per region ------------------------------------------------------------------------
def _case_rays(name, T, N=36):
    """region 0 (32 x 32) holds exactly T distinct rays, every other region fewer"""
    rng = np.random.default_rng(1000 + T)
    seq = _regions(N)
    m = T + 37
    rows = {}
    r0 = seq[0]
    for k, s in enumerate(r0):
        own = np.arange(k, T, r0.size)                # ray t sits in row t mod 1024: every ray below T is met
        extra = _pick(rng, T, int(rng.integers(6, 14)))
        rays = np.union1d(own, extra)
        rows[int(s)] = (rays, _ids(rng, rays.size, "skew"))
    for g in (1, 2, 3):
        _background(rng, rows, seq[g], np.arange(T // 2, m), 4, 12)
    return Case(name, N, m, rows, f"region 0 holds {T} rays")


def _case_no_plan(name):
    """a 16 x 16 region (the corner tile columns of N = 36 are only 4 wide, so the first 16 x 16 block) of
    2,048 distinct rays: no LDS shape at R = 32 nor at R = 16"""
    N = 36
    reg16, nreg16 = row_regions(N, 16)
    block = region_rows(reg16, nreg16)[0]
    assert block.size == 256
    rows = {}
    rng = np.random.default_rng(77)
    for k, s in enumerate(block):
        rows[int(s)] = (np.arange(8 * k, 8 * k + 8), _ids(rng, 8, "skew"))
    return Case(name, N, 2048 + 37, rows, "2,048 rays in one 16 x 16 region")


# --- B: row lengths and pair spans ----------------------------------------------------------------
def _case_lengths(name, longest, N=40):
    """the crafted units in the first run of region 0 (stored rows 0..), longest row `longest`"""
    K = constants()
    rng = np.random.default_rng(500 + longest)
    seq = _regions(N)
    m = 293
    q = _Seq(K["CHUNK"])
    k = 37
    for parity in (0, 1):
        for span in (K["CHUNK"] - 1, K["CHUNK"], K["CHUNK"] + 1):
            a = 60 + parity
            q.unit(a, span - parity - a, parity)
    for a, b in ((0, k), (k, 0), (0, 0), (1, 1), (63, 64), (64, 64), (1, 127)):
        q.unit(a, b, 0)
    q.unit(100, 100, 0)                              # cut after the first 100 ...
    q.row(100)                                       # ... and after the second: a run of a single row
    q.unit(5, 6, 1)
    if longest != 127:
        q.unit(longest, None, 0)                     # (alone: 128 and more turn the pairs off or refuse the plan)
        q.row(3)
    lens = q.lens
    assert len(lens) <= 120 and max(lens) == longest
    rows = {}
    for s, L in zip(seq[0], lens):
        rows[int(s)] = (_pick(rng, m, L), _ids(rng, L, "skew"))
    _background(rng, rows, seq[0][len(lens):], m, 18, 40)
    for g in (1, 2, 3):
        _background(rng, rows, seq[g], m, 10, 30)
    return Case(name, N, m, rows, f"crafted units, longest row {longest}")


# --- C: wave shares and empties -----------------------------------------------------------------
def _case_shares(name, variant, N=36):
    rng = np.random.default_rng(800 + variant)
    seq = _regions(N)
    m = 411
    rows = {}
    if variant == 1:
        # region 1: everything in its first stored row; region 2: in its last; region 3 (the last): empty,
        # and its rows end the CSR
        rows[int(seq[1][0])] = (_pick(rng, m, 90), _ids(rng, 90, "skew"))
        rows[int(seq[2][-1])] = (_pick(rng, m, 77), _ids(rng, 77, "skew"))
        for g in (1, 2, 3):
            for s in seq[g]:
                rows.setdefault(int(s), (np.empty(0, int), np.empty(0, int)))
        _background(rng, rows, seq[0], m, 10, 40)
    else:
        # region 1: empty; the last stored row (region 3) is the longest, at an odd entry, nnz odd
        for s in seq[1]:
            rows[int(s)] = (np.empty(0, int), np.empty(0, int))
        last = int(seq[3][-1])
        assert last == N * N - 1
        rows[last] = (_pick(rng, m, 126), _ids(rng, 126, "skew"))
        _background(rng, rows, seq[0], m, 10, 40)
        _background(rng, rows, seq[2], m, 10, 40)
        _background(rng, rows, seq[3], m, 10, 40)
        before = sum(len(rows[s][0]) for s in rows if s != last)
        if before % 2 == 0:                            # the last row starts at an odd entry
            s = int(seq[0][5])
            rows[s] = (rows[s][0][:-1], rows[s][1][:-1])
    return Case(name, N, m, rows, "wave shares and empty regions %d" % variant)


# --- D: runs per wave ------------------------------------------------------------------------------
def _case_runs(name, want, N=36):
    """rows of 100 entries in a row cut their run after every row: k of them at the head of region 0 give
    its first wave k runs (and one more for the rows behind them)"""
    K = constants()
    seq = _regions(N)
    m = 301
    for k in range(want - 4, want + 4):
        rng = np.random.default_rng(900 + want)
        rows = {}
        for s in seq[0][:k]:
            rows[int(s)] = (_pick(rng, m, 100), _ids(rng, 100, "skew"))
        _background(rng, rows, seq[0][k:], m, 28, 36)
        for g in (1, 2, 3):
            _background(rng, rows, seq[g], m, 8, 20)
        c = Case(name, N, m, rows, f"{want} runs in the fullest wave")
        bv = c.bview()
        reg, nreg = row_regions(N, K["REGION"])
        cut = [pair_cuts(r, bv.rp, K["CHUNK"]) for g in range(nreg) for r in wave_shares(region_rows(reg, nreg)[g], bv.rp)]
        if max(len(r) for r in cut) == want:
            return c
    raise AssertionError(name)


# --- E: ray multiplicity and range -----------------------------------------------------------------
E_M = 517
E_GAP = (190, 330)                                   # rays [190, 330) meet no pixel: bands 3 and 4 are empty
E_ALL, E_ONE = 100, 400


def _case_rays_multi(name, ends, N=36):
    """ray E_ALL in one pixel of every region, ray E_ONE in exactly one pixel, rays E_GAP nowhere; rays 0 and
    m - 1 present (`ends`) or absent"""
    rng = np.random.default_rng(300 + ends)
    seq = _regions(N)
    pool = np.setdiff1d(np.arange(1, E_M - 1), np.r_[np.arange(*E_GAP), E_ALL, E_ONE])
    rows = {}
    _background(rng, rows, np.arange(N * N), pool, 10, 30)
    def add(s, ray, vid):
        rays, ids = rows[int(s)]
        at = int(np.searchsorted(rays, ray))
        assert at == rays.size or rays[at] != ray
        rows[int(s)] = (np.insert(rays, at, ray), np.insert(ids, at, vid))

    if ends:
        add(seq[0][3], 0, 0)
        add(seq[2][7], E_M - 1, 0)
    for g in range(4):
        add(seq[g][len(seq[g]) // 2], E_ALL, 1)
    add(seq[0][11], E_ONE, 2)
    return Case(name, N, E_M, rows, "ray multiplicities, ends %s" % ("present" if ends else "absent"))


def _case_one_row(name, N=36):
    rng = np.random.default_rng(31)
    s = int(_regions(N)[0][517])
    return Case(name, N, 203, {s: (_pick(rng, 203, 50), _ids(rng, 50, "skew"))}, "a single non-empty pixel row")


# --- F: values for the compact stream --------------------------------------------------------------
SUB_RAYS = 60                                        # rays [0, 60) carry the stored subnormals
def _case_values(name, kind, N=36):
    rng = np.random.default_rng(600 + len(kind))
    seq = _regions(N)
    m = 301
    rows = {}
    if kind == "mixed":
        # units at the head of region 0's first run: (fully coded, fully escaped), (escaped, coded), first
        # rows with an odd and an even number of coded entries; escapes are ids >= 1000 (each used once)
        nxt = [1000]

        def esc(L):
            out = np.arange(nxt[0], nxt[0] + L)
            nxt[0] += L
            return out

        def cod(L):
            return rng.integers(0, 8, L)

        plan = [(cod(30), esc(33)), (esc(28), cod(31)), (np.r_[cod(7), esc(20)], np.r_[cod(9), esc(4)]),
                (np.r_[esc(11), cod(12)], np.r_[esc(3), cod(3)])]
        for (a, b), s in zip(plan, seq[0][0:8:2]):
            for ids, t in ((a, s), (b, s + 1)):
                rows[int(t)] = (_pick(rng, m, ids.size), rng.permutation(ids))
        _background(rng, rows, np.arange(N * N), m, 20, 44, "few")
    elif kind == "zeros":
        # +0.0, -0.0 and a subnormal are the three most frequent stored bit patterns
        _background(rng, rows, np.arange(N * N), m, 20, 44, "few")
        for s in list(rows):
            rays, ids = rows[s]
            ids = np.array(ids)
            u = rng.random(ids.size)
            ids[u < 0.12] = ZERO_P
            ids[(u >= 0.12) & (u < 0.21)] = ZERO_M
            ids[(rays < SUB_RAYS) & (u >= 0.5)] = SUBNORMAL    # (half of a ray's entries: its sums stay normal)
            rows[s] = (rays, ids)
    else:
        _background(rng, rows, np.arange(N * N), m, 20, 44, {"codes31": "few", "skew40": "skew", "distinct": "skew"}[kind])
        if kind == "distinct":
            k = 0
            for s in sorted(rows):
                rays, _ = rows[s]
                rows[s] = (rays, np.arange(k, k + rays.size))
                k += rays.size
    return Case(name, N, m, rows, "values: " + kind)


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
def ray_targets():
    S = constants()["SHAPES"]
    return [t for s in S for t in (s - 64, s - 64 + 1)]


def vstream_targets():
    """(slots, c, rays): the fullest region leaves c free slots under the dummies' neighbour, or none (-1)"""
    return [(s, c, s - 65 - c if c >= 0 else s - 64) for s in constants()["SHAPES"] for c in (31, 30, 1, 0, -1)]


def case_names():
    names = ["codes31", "skew40", "distinct", "mixed", "zeros",                      # F
             "ends_present", "ends_absent", "one_row"]                                # E
    names += ["len127", "len128", "len255", "len256"]                                 # B
    names += ["shares1", "shares2"]                                                   # C
    names += ["runs64", "runs65"]                                                     # D
    names += ["rays%d" % t for t in ray_targets()] + ["no_plan"]                      # A
    names += ["vs%d_%d" % (s, r) for s, _, r in vstream_targets()]
    return names


@functools.lru_cache(maxsize=None)
def case(name):
    if name in ("codes31", "skew40", "distinct", "mixed", "zeros"):
        return _case_values(name, name)
    if name in ("ends_present", "ends_absent"):
        return _case_rays_multi(name, name == "ends_present")
    if name == "one_row":
        return _case_one_row(name)
    if name.startswith("len"):
        return _case_lengths(name, int(name[3:]))
    if name.startswith("shares"):
        return _case_shares(name, int(name[6:]))
    if name.startswith("runs"):
        return _case_runs(name, int(name[4:]))
    if name == "no_plan":
        return _case_no_plan(name)
    if name.startswith("rays"):
        return _case_rays(name, int(name[4:]))
    if name.startswith("vs"):
        return _case_rays(name, int(name.split("_")[1]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def plan_of(name, mode="real", dtype=0, rowpair=4, vstream=0, shard=None):
    bv = view_of(name, mode, dtype, shard)
    return twin_plan(bv, rowpair=rowpair, vstream=vstream if dtype == 0 else 0, es=8 if dtype == 0 else 4)


@functools.lru_cache(maxsize=None)
def view_of(name, mode="real", dtype=0, shard=None):
    bv = case(name).bview(mode, dtype)
    return bv if shard is None else bv.shard(*shard)


# ---------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------
UNIT = {0: 2.0 ** -53, 1: 2.0 ** -24}
# half the spacing of the subnormals: the absolute error of a product that underflows (sums of subnormals are
# exact); it matters only where a stored subnormal is all a sum holds (case "zeros" under a unit vector)
ETA = {0: np.longdouble(2.0) ** -1075, 1: np.longdouble(2.0) ** -150}
WIDE_OK = np.finfo(np.longdouble).eps < 2.0 ** -53 and np.finfo(np.longdouble).minexp < -4000
LD_EPS = float(np.finfo(np.longdouble).eps)


def _gamma(k, u):
    k = k * u
    return k / (1.0 - k)


class Reference:
    """Bq (stored row order of the view) and A(Bq) in np.longdouble from inputs rounded to the operator's
    type, with the bounds of a product in any summation order: |Bq_j - ref| <= gamma(L_j + 1) (|B||q|)_j and
    |A(Bq)_i - ref| <= gamma(La_i + Lb*_i + 2) (|A||B||q|)_i, Lb*_i the longest pixel row on ray i.  To each
    comes the reference's own rounding and eta per product for underflow (the standard model's absolute term:
    L_j eta, and (La_i + sum_j |A_ij| L_j) eta)."""

    def __init__(self, bv, q, dtype):
        assert WIDE_OK
        self.dtype, self.bv = dtype, bv
        ld = np.longdouble
        val = bv.val.astype(ld)
        qv = np.asarray(q, dtype=np.float64)
        if dtype == 1:
            qv = qv.astype(np.float32).astype(np.float64)
        qv = qv.astype(ld)
        t = val * qv[bv.ci]
        self.bq = np.zeros(bv.rows, dtype=ld)
        self.sbq = np.zeros(bv.rows, dtype=ld)
        np.add.at(self.bq, bv.rowidx, t)
        np.add.at(self.sbq, bv.rowidx, np.abs(t))
        self.abq = np.zeros(bv.m, dtype=ld)
        self.sab = np.zeros(bv.m, dtype=ld)
        np.add.at(self.abq, bv.ci, val * self.bq[bv.rowidx])
        np.add.at(self.sab, bv.ci, np.abs(val) * self.sbq[bv.rowidx])
        self.L = bv.len.astype(np.int64)
        self.La = np.bincount(bv.ci, minlength=bv.m).astype(np.int64)
        self.Lb = np.zeros(bv.m, dtype=np.int64)
        np.maximum.at(self.Lb, bv.ci, self.L[bv.rowidx])
        u, eta = UNIT[dtype], ETA[dtype]
        carried = np.zeros(bv.m, dtype=ld)
        np.add.at(carried, bv.ci, np.abs(val) * self.L[bv.rowidx])
        self.bound_bq = (_gamma(self.L + 1.0, u) + (self.L + 1) * LD_EPS).astype(ld) * self.sbq + self.L * eta
        self.bound_ab = ((_gamma(self.La + self.Lb + 2.0, u) + (self.La + self.Lb + 2) * LD_EPS).astype(ld) * self.sab +
                         (self.La + carried) * eta)

    def check(self, bq, abq, what=""):
        """asserts the bounds; returns the largest ratios (Bq, A(Bq)) to them"""
        out = []
        for got, ref, bound, L, tag in ((bq, self.bq, self.bound_bq, self.L, "Bq"), (abq, self.abq, self.bound_ab, self.La, "A(Bq)")):
            got = np.asarray(got, dtype=np.float64)
            assert got.shape == ref.shape, (what, tag, got.shape)
            assert np.all(np.isfinite(got)), (what, tag, "not written", np.flatnonzero(~np.isfinite(got))[:8])
            empty = L == 0
            assert np.all(got[empty] == 0.0), (what, tag, "empty not 0", np.flatnonzero(empty & (got != 0))[:8])
            err = np.abs(got.astype(np.longdouble) - ref)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0)).astype(np.float64)
            r = float(ratio.max(initial=0.0))
            assert r <= 1.0, (what, tag, "derived bound", r, int(np.argmax(ratio)))
            out.append(r)
        return tuple(out)


def exact_products(bv, q):
    """(Bq, A(Bq), the largest numerators of |B||q| * 16 and |A||B||q| * 256) in integer arithmetic: values k/16
    (special values count as 0: +-0.0 are, and q is 0 on every ray that carries the subnormal), q integers"""
    k16 = bv.val * 16.0
    sub = np.abs(bv.val) == SPECIAL[SUBNORMAL]
    k16 = np.where(sub, 0.0, k16)
    assert np.all(k16 == np.round(k16)) and np.all(q == np.round(q))
    k = k16.astype(np.int64)
    qi = np.asarray(q).astype(np.int64)
    bq = np.zeros(bv.rows, dtype=np.int64)
    sbq = np.zeros(bv.rows, dtype=np.int64)
    np.add.at(bq, bv.rowidx, k * qi[bv.ci])
    np.add.at(sbq, bv.rowidx, np.abs(k * qi[bv.ci]))
    ab = np.zeros(bv.m, dtype=np.int64)
    sab = np.zeros(bv.m, dtype=np.int64)
    np.add.at(ab, bv.ci, k * bq[bv.rowidx])
    np.add.at(sab, bv.ci, np.abs(k) * sbq[bv.rowidx])
    return bq / 16.0, ab / 256.0, int(sbq.max(initial=0)), int(sab.max(initial=0))


def subnormal_rays(bv):
    """rays that carry a stored subnormal (their A(Bq) is not an exact sum), and the pixels on them"""
    sub = np.abs(bv.val) == SPECIAL[SUBNORMAL]
    return np.unique(bv.ci[sub]), np.unique(bv.rowidx[sub])


def exact_qs(bv, dtype, extra_units=()):
    """[(label, q)]: ones, random integers, unit vectors on the first and last hit ray, an empty ray (if any)
    and `extra_units`; all 0 on the rays that carry a subnormal"""
    rng = np.random.default_rng(11)
    hi = 3 if dtype == 0 else 1
    hit = np.zeros(bv.m, dtype=bool)
    hit[bv.ci] = True
    rays = np.flatnonzero(hit)
    qs = [("ones", np.ones(bv.m)), ("integers", rng.integers(-hi, hi + 1, bv.m).astype(np.float64))]
    units_ = [("first hit ray", int(rays[0])), ("last hit ray", int(rays[-1]))] if rays.size else []
    if (~hit).any():
        units_.append(("empty ray", int(np.flatnonzero(~hit)[0])))
    units_ += list(extra_units)
    for label, i in units_:
        e = np.zeros(bv.m)
        e[i] = 1.0
        qs.append((label, e))
    mask = np.ones(bv.m)
    mask[subnormal_rays(bv)[0]] = 0.0
    return [(label, q * mask) for label, q in qs]
