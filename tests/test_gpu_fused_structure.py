"""The one-pass A*(B*q) row-wave plan and kernel at their structure edges (csrc/fused.hip: fused_plan_build_rw,
fused_plan_dev_finish, fused_plan_vstream, k_fused_rw).

The operators are those of fused_cases.py: prescribed patterns over a 36^2 or 40^2 grid in 4 x 4 tiles
(regions of 1024 / 128 / 128 / 16 and 1024 / 256 / 256 / 64 pixel rows at the default region side), built
row by row in the stored order so that each sits on one edge of the plan:

  A  the fullest region holds exactly MAXR - 64 and MAXR - 64 + 1 rays for every LDS shape (the last one
     sends the plan to 16 x 16 regions), 2,048 rays in one 16 x 16 region (no plan), and MAXR - 65 - c rays
     for c = 31, 30, 1, 0, -1 with the compact stream (all codes, a cut dictionary, one code, none, plain);
  B  units whose span len + len + (rp & 1) is 127, 128, 129 at both parities, rows of 0/k, k/0, 0/0, 1/1,
     63/64, 64/64, 1/127 entries, an odd run, a run of one row; a longest row of 127, 128 (single rows), 255
     (two chunks) and 256 (refused);
  C  a region with all its entries in its first row, one with all in its last, an empty region, an empty
     last region, empty rows at the end of the CSR, and a longest last row at an odd entry with nnz odd (the
     chunk load reads into lidx's padding);
  D  exactly 64 and 65 runs in the fullest wave after the pair cuts;
  E  a ray in every region, a ray in one pixel, rays 0 and m - 1 present and absent, 140 consecutive rays
     that meet no pixel, m no multiple of 32, a single non-empty pixel row;
  F  at most 31 distinct values, 40 with a skewed frequency, all distinct, fully coded next to fully
     escaped rows, odd and even c0h, and +0.0, -0.0 and a subnormal as the most frequent stored patterns;
  G  the two tile-column shards of B's 40^2 case.

The CPU tests (unmarked) prove each property with the twin of the plan rules.  The GPU tests assert the path
taken (fused_plan_info and the plan's own HGM_FUSED_VERBOSE report against the twin) and hold every product
to a reference of its own, into NaN-filled outputs:

  exact   values k/16 and integer q: every partial sum of both products is representable (asserted from
          |A||B||q|), so Bq and A(Bq) equal the integer result in every summation order: no tolerance;
  real    normal values and q, the sums in np.longdouble, |Bq_j - ref| <= gamma(L_j + 1)(|B||q|)_j and
          |A(Bq)_i - ref| <= gamma(La_i + Lb*_i + 2)(|A||B||q|)_i (gamma(k) = k u / (1 - k u)), empty rows and
          rays exactly 0 (plus the standard model's underflow term per product, fused_cases.Reference: it
          is felt only where a stored subnormal is all a sum holds);
  bits    a repeated call, fused_reduce 0 / 1, fused_plan_dev 0 / 1 (equal checksums), fused_vsdepth 2 / 3,
          compact (3 and 2) against plain on unit vectors, a refused plan against fused_ab = 0;

each under fused_rowpair = 4 with fused_vstream = 0 and 3, fused_rowpair = 0, and fp32 operators.  Three
Golub-Kahan iterations (lsqr_solver, lsmr_solver; fp64 and fp32) run on cases B and C against the two-pass
solve and the oracle at the bars of test_gpu_fused.py / test_gpu_lengths.py.  The largest ratios to the
derived bounds are printed by every test (run with -s)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import scipy.sparse as sp

import hgmres
from hgmres import _lib as L
from hgmres.dist import tile_column_shards
from oracle import restatement as R   # checker only
import fused_cases as FC
from test_gpu_fused import _Rounded32

gpu = pytest.mark.gpu

K = FC.constants()
SHAPES, CHUNK, CAP, CODES = K["SHAPES"], K["CHUNK"], K["RUN_CAP"], K["VS_CODES"]
FT = {0: np.float64, 1: np.float32}
NAMES = FC.case_names()
SHARDS = [("len127", s) for s in tile_column_shards(40, 2, FC.TILE)]
# (option set) -> (dtype, options, the twin's arguments)
OPTSETS = {"rp4": (0, dict(fused_rowpair=4, fused_vstream=0), dict(rowpair=4, vstream=0)),
           "rp4vs3": (0, dict(fused_rowpair=4, fused_vstream=3), dict(rowpair=4, vstream=3)),
           "rp0": (0, dict(fused_rowpair=0), dict(rowpair=0, vstream=1)),
           "f32": (1, dict(), dict(rowpair=4, vstream=1))}
# the mildest cases first (F, E), the sharpest last (C, D, A)
TARGETS = [(n, None) for n in NAMES[:12]] + SHARDS + [(n, None) for n in NAMES[12:]]
TARGET_IDS = [n if s is None else f"{n}[{s[0]}:{s[1]}]" for n, s in TARGETS]


def _twin(name, optset, mode="real", shard=None):
    dtype, _, kw = OPTSETS[optset]
    return FC.plan_of(name, mode, dtype, kw["rowpair"], kw["vstream"], shard)


# ---------------------------------------------------------------------------------------------
# CPU: the constants, the twin and every case's named property
# ---------------------------------------------------------------------------------------------
def test_constants_read_from_csrc():
    assert K["RW_ROW_MAX"] == 255 and K["RW_SLOTS_MAX"] == 4096 and SHAPES == (1088, 1344, 1536, 2048)
    assert CODES == 31 and CHUNK == 128 and CAP == 64 and K["REGION"] == 32 and K["LIDX_PAD"] == 256
    assert K["PLAN_DEV_MAX_M"] == 19 * 1024 * 32
    assert max(FC.case(n).m for n in NAMES) <= K["PLAN_DEV_MAX_M"]     # (every case takes the device build)


def test_grids_and_regions():
    for N, sizes in ((36, [1024, 128, 128, 16]), (40, [1024, 256, 256, 64])):
        reg, nreg = FC.row_regions(N, K["REGION"])
        assert nreg == 4 and [int((reg == g).sum()) for g in range(4)] == sizes
    # a shard of whole tile columns numbers its rows as the grid does, from its own first column
    inv = np.empty(1600, dtype=np.int64)
    inv[FC.stored_pixel_index(40)] = np.arange(1600)
    for lo, hi in tile_column_shards(40, 2, FC.TILE):
        sreg, snreg = FC.row_regions(40, 16, hi - lo)
        p = inv[lo:hi]
        r, c = p % 40, p // 40 - lo // 40
        assert snreg == 3 * 2 and c.min() == 0 and c.max() == 19
        assert np.array_equal(sreg, (c // 16) * 3 + r // 16), (lo, hi)


def test_twin_rules_on_a_hand_example():
    rp = np.array([0, 3, 3, 130, 131, 131, 200])
    # 200 entries: row 2 (127 entries) ends the first share, the second is passed over
    assert FC.wave_shares(np.arange(6), rp) == [[[0, 3]], [], [[3, 3]], []]
    assert FC.wave_shares(np.array([0, 1, 4, 5]), rp)[0] == [[0, 2], [4, 2]]
    # rows 2, 3: 127 + 1 entries from an odd entry: 129, cut after row 2
    assert not FC.pair_fits(rp, 2, CHUNK) and FC.pair_fits(rp, 0, CHUNK)
    assert FC.pair_cuts([[0, 6]], rp, CHUNK) == [[0, 3], [3, 3]]
    assert FC.pair_cuts([[2, 2]], rp, CHUNK) == [[2, 1], [3, 1]]
    d = FC.value_dictionary(np.array([1.0, 1.0, 2.0, 0.0, 0.0, 0.0, 5e-324, 5e-324, 3.0, 3.0, 3.0]), 31)
    assert sorted(d.view(np.float64).tolist()) == [1.0, 3.0]
    assert FC.value_dictionary(np.array([1.0, 1.0, 3.0, 3.0, 3.0]), 1).view(np.float64).tolist() == [3.0]


@pytest.mark.parametrize("name", NAMES)
def test_case_sizes(name):
    c = FC.case(name)
    S = c.matrix()
    assert S.shape == (c.m, c.N ** 2) and c.N in (36, 40) and S.nnz <= 3e5 and c.m % 32 and c.m % 64
    assert S.has_sorted_indices or S.nnz == 0
    bv = c.bview()
    assert bv.nnz == S.nnz and np.all(np.diff(bv.rp) >= 0)
    for s in range(bv.rows):                            # rays ascend inside a pixel row: no repeated entry
        assert np.all(np.diff(bv.ci[bv.rp[s]:bv.rp[s + 1]]) > 0)


# --- A -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", SHAPES)
def test_case_a_rays_per_region(slots):
    full, over = slots - 64, slots - 63
    p = _twin("rays%d" % full, "rp4")
    assert p["count"][0] == full == p["worst"] and max(p["count"][1:]) < full
    assert p["slots"] == slots and p["region"] == 32 and not p["refused"] and p["rowpair"]
    q = _twin("rays%d" % over, "rp4")
    nxt = [s for s in SHAPES if s > slots]
    if nxt:
        assert q["worst"] == over and q["slots"] == nxt[0] and q["region"] == 32
    else:                                               # 1,985 rays: the plan is retried at R = 16
        at32 = FC._plan_at(FC.view_of("rays%d" % over), 32, 4, 8)
        assert at32["refused"] == "lds" and at32["worst"] == over
        assert q["region"] == 16 and q["tried"] == 2 and not q["refused"] and q["worst"] <= SHAPES[-1] - 64


def test_case_a_no_plan():
    p = _twin("no_plan", "rp4")
    assert p["refused"] == "lds" and p["region"] == 16 and p["worst"] == 2048 > SHAPES[-1] - 64
    reg16, n16 = FC.row_regions(36, 16)
    bv = FC.view_of("no_plan")
    assert np.unique(reg16[bv.rowidx]).size == 1        # all of it in one 16 x 16 region


@pytest.mark.parametrize("slots,c,rays", FC.vstream_targets())
def test_case_a_compact_room(slots, c, rays):
    name = "vs%d_%d" % (slots, rays)
    p = _twin(name, "rp4vs3")
    assert p["worst"] == rays and p["slots"] == slots and p["rowpair"]
    ncand = FC.value_dictionary(FC.view_of(name).val, 99).size
    assert ncand >= CODES                               # the values would fill the dictionary: the room cuts it
    if c < 0:
        assert not p["compact"] and _twin(name, "rp4")["slots"] == slots
    else:
        assert p["compact"] and p["codes"] == min(c, CODES) and slots - 65 - p["codes"] >= rays
        assert (c, p["codes"]) in ((31, 31), (30, 30), (1, 1), (0, 0))


# --- B -------------------------------------------------------------------------------------------
def test_case_b_units():
    bv = FC.view_of("len127")
    p = _twin("len127", "rp4")
    assert p["rowpair"] and p["maxlen"] == 127 and not p["refused"]
    us = FC.units(bv, p)
    pairs = {(u["span"], u["parity"]) for u in us if not u["single"]}
    for parity in (0, 1):
        assert (CHUNK - 1, parity) in pairs and (CHUNK, parity) in pairs, parity
        # 129: the first row alone at the end of its run, the second opens the next run
        cut = [i for i, u in enumerate(us) if u["single"] and u["parity"] == parity and u["row"] + 1 < bv.rows and
               u["lenA"] + bv.len[u["row"] + 1] + parity == CHUNK + 1 and us[i + 1]["row"] == u["row"] + 1]
        assert cut, parity
    assert max(s for s, _ in pairs) == CHUNK
    k = 37
    lens = {(u["lenA"], u["lenB"]) for u in us if not u["single"]}
    assert {(0, k), (k, 0), (0, 0), (1, 1), (63, 64), (64, 64), (1, 127)} <= lens
    runs = [r for w in p["wave_runs"] for r in w]
    assert any(y % 2 == 1 and y > 1 for _, y in runs) and any(y == 1 for _, y in runs)
    assert max(p["runs_per_wave"]) <= CAP


def test_case_b_longest_rows():
    base = FC.view_of("len127")
    for name, maxlen in (("len128", 128), ("len255", 255), ("len256", 256)):
        bv = FC.view_of(name)
        assert bv.len.max() == maxlen and np.count_nonzero(bv.len == maxlen) == 1
        assert np.count_nonzero(bv.len > 127) == 1 and base.len.max() == 127
        for optset in OPTSETS:
            p = _twin(name, optset)
            assert not p["rowpair"] and p["refused"] == ("row" if maxlen == 256 else None), (name, optset)
    assert _twin("len127", "rp4")["rowpair"] and _twin("len127", "f32")["rowpair"] and not _twin("len127", "rp0")["rowpair"]


# --- C -------------------------------------------------------------------------------------------
def test_case_c_shares_and_empties():
    bv = FC.view_of("shares1")
    p = _twin("shares1", "rp4")
    rows = FC.region_rows(p["reg"], 4)
    assert bv.len[rows[1][0]] == bv.len[rows[1]].sum() == 90        # region 1: all in its first stored row
    assert bv.len[rows[2][-1]] == bv.len[rows[2]].sum() == 77       # region 2: all in its last
    per = lambda g: p["runs_per_wave"][4 * g:4 * g + 4]   # noqa: E731
    assert per(1)[1] == per(1)[2] == 0 and per(1)[0] == 1 and per(1)[3] >= 1
    assert per(2)[1:] == [0, 0, 0] and per(2)[0] >= 1
    assert p["count"][3] == 0 and bv.len[rows[3]].sum() == 0         # the last region: nr = 0
    assert np.array_equal(rows[3], np.arange(bv.rows - 16, bv.rows)) and bv.rp[-17] == bv.nnz   # trailing empty rows
    bv = FC.view_of("shares2")
    p = _twin("shares2", "rp4")
    rows = FC.region_rows(p["reg"], 4)
    assert p["count"][1] == 0 and p["count"][3] > 0 and p["rowpair"]
    last = bv.rows - 1
    assert bv.len[last] == bv.len.max() == 126 and np.count_nonzero(bv.len == 126) == 1
    assert bv.rp[last] % 2 == 1 and bv.nnz % 2 == 1
    # the chunk of the last unit is read from the even entry below its first row: it ends past nnz
    u = [u for u in FC.units(bv, p) if u["row"] <= last < u["row"] + (1 if u["single"] else 2)][0]
    assert (bv.rp[u["row"]] & ~1) + CHUNK > bv.nnz and (bv.rp[u["row"]] & ~1) + CHUNK <= bv.nnz + K["LIDX_PAD"]


# --- D -------------------------------------------------------------------------------------------
def test_case_d_runs_per_wave():
    p = _twin("runs64", "rp4")
    assert p["rowpair"] and max(p["runs_per_wave"]) == CAP and not p["refused"]
    bv = FC.view_of("runs65")
    reg, nreg = FC.row_regions(36, 32)
    cut = [FC.pair_cuts(r, bv.rp, CHUNK) for g in range(nreg) for r in FC.wave_shares(FC.region_rows(reg, nreg)[g], bv.rp)]
    assert max(len(r) for r in cut) == CAP + 1 and bv.len.max() <= 127
    p = _twin("runs65", "rp4")
    assert not p["rowpair"] and not p["refused"] and max(p["runs_per_wave"]) < CAP
    assert not _twin("runs65", "rp4vs3")["compact"] and _twin("runs64", "rp4vs3")["compact"]


# --- E -------------------------------------------------------------------------------------------
def test_case_e_rays():
    for name, ends in (("ends_present", True), ("ends_absent", False)):
        bv = FC.view_of(name)
        p = _twin(name, "rp4")
        hit = np.bincount(bv.ci, minlength=bv.m)
        assert bv.m == FC.E_M and bv.m % 32 and bv.m % 64
        assert (hit[0] > 0) == ends and (hit[-1] > 0) == ends
        assert np.all(hit[FC.E_GAP[0]:FC.E_GAP[1]] == 0) and FC.E_GAP[1] - FC.E_GAP[0] >= 130
        band = np.arange(-(-FC.E_GAP[0] // 64) * 64, -(-FC.E_GAP[0] // 64) * 64 + 64)
        assert band[0] >= FC.E_GAP[0] and band[-1] < FC.E_GAP[1]          # a whole 64-ray band is empty
        assert hit[FC.E_ONE] == 1 and hit[FC.E_ALL] == 4
        assert sorted(p["reg"][bv.rowidx[bv.ci == FC.E_ALL]].tolist()) == [0, 1, 2, 3]
        assert all(FC.E_ALL in r for r in p["rays"])
    bv = FC.view_of("one_row")
    assert np.count_nonzero(bv.len) == 1 and bv.nnz == 50
    assert not _twin("one_row", "rp4")["refused"]


# --- F -------------------------------------------------------------------------------------------
def test_case_f_values():
    def bits(name):
        return np.unique(FC.view_of(name).val.view(np.uint64), return_counts=True)

    u, c = bits("codes31")
    assert u.size <= CODES and c.min() >= 2
    p = _twin("codes31", "rp4vs3")
    assert p["compact"] and p["codes"] == u.size and p["coded"].all()
    u, c = bits("skew40")
    assert u.size == 40 and c.max() > 50 * c.min() and c.min() >= 2
    p = _twin("skew40", "rp4vs3")
    assert p["compact"] and p["codes"] == CODES and 0.9 < p["coded"].mean() < 1.0
    u, c = bits("distinct")
    assert c.max() == 1
    p = _twin("distinct", "rp4vs3")
    assert p["compact"] and p["codes"] == 0                     # (the measurement form: every value an escape)
    assert not FC.plan_of("distinct", "real", 0, 4, 1)["compact"]       # the default keeps the plain plan
    assert FC.plan_of("codes31", "real", 0, 4, 1)["compact"]            # (and takes the compact one here)
    # mixed: fully coded / fully escaped partners in both orders, odd and even coded counts in first rows
    bv = FC.view_of("mixed")
    p = _twin("mixed", "rp4vs3")
    us = [u for u in FC.units(bv, p, p["coded"]) if not u["single"]]
    assert any(u["codedA"] == u["lenA"] > 0 and u["codedB"] == 0 < u["lenB"] for u in us)
    assert any(u["codedB"] == u["lenB"] > 0 and u["codedA"] == 0 < u["lenA"] for u in us)
    mixed = [u for u in us if 0 < u["codedA"] < u["lenA"]]
    assert any(u["codedA"] % 2 == 1 for u in mixed) and any(u["codedA"] % 2 == 0 for u in mixed)
    assert {u["c0h"] for u in us} >= {0, 3, 6, 15}
    # zeros: the three most frequent stored patterns, none of them a code
    bv = FC.view_of("zeros")
    u, c = bits("zeros")
    top = set(u[np.argsort(-c)[:3]].tolist())
    special = {int(np.array(v).view(np.uint64)) for v in FC.SPECIAL.values()}
    assert top == special and np.signbit(FC.SPECIAL[FC.ZERO_M]) and 0 < FC.SPECIAL[FC.SUBNORMAL] < np.finfo(float).tiny
    p = _twin("zeros", "rp4vs3")
    assert p["compact"] and not (set(p["code_bits"].tolist()) & special) and p["codes"] == 16
    rays, _ = FC.subnormal_rays(bv)
    assert np.array_equal(rays, np.arange(FC.SUB_RAYS))
    for i in rays:                                      # (the sums of a ray with subnormals stay normal)
        assert np.count_nonzero(np.abs(bv.val[bv.ci == i]) > 1e-3) >= 5


# --- G -------------------------------------------------------------------------------------------
def test_case_g_shards():
    (lo0, hi0), (lo1, hi1) = [s for _, s in SHARDS]
    assert lo0 == 0 and hi0 == lo1 == 800 and hi1 == 1600
    whole = FC.view_of("len127")
    for name, (lo, hi) in SHARDS:
        bv = FC.view_of(name, shard=(lo, hi))
        assert bv.rows == hi - lo and np.array_equal(bv.len, whole.len[lo:hi])
        p = _twin(name, "rp4", shard=(lo, hi))
        assert not p["refused"] and p["rowpair"] and p["nreg"] == 2 and sorted(map(len, FC.region_rows(p["reg"], 2))) == [160, 640]


# --- exact inputs ----------------------------------------------------------------------------------
def _unit_rays(name, bv):
    if name.startswith("ends_"):
        return [("every-region ray", FC.E_ALL), ("one-pixel ray", FC.E_ONE), ("ray in the empty stretch", FC.E_GAP[0] + 70)]
    return []


@pytest.mark.parametrize("dtype", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("name,shard", TARGETS, ids=TARGET_IDS)
def test_exact_inputs_are_exact(name, shard, dtype):
    """every partial sum of |A||B||q| has a numerator below 2^53 (2^24): the products are exact in any order"""
    bv = FC.view_of(name, "exact", dtype, shard)
    k16 = np.where(np.abs(bv.val) == FC.SPECIAL[FC.SUBNORMAL], 0.0, bv.val * 16)
    assert np.all(k16 == np.round(k16)) and np.abs(k16).max() <= 20
    for label, q in FC.exact_qs(bv, dtype, _unit_rays(name, bv)):
        _, _, nbq, nab = FC.exact_products(bv, q)
        lim = 2 ** 53 if dtype == 0 else 2 ** 24
        assert nbq < lim and nab < lim, (name, label, nbq, nab)
    if name == "ends_present":
        assert len(FC.exact_qs(bv, dtype, _unit_rays(name, bv))) == 8


def test_reference_rejects_what_a_wrong_kernel_would_give():
    bv = FC.view_of("shares1")
    q = np.random.default_rng(3).standard_normal(bv.m)
    for dtype in (0, 1):
        ref = FC.Reference(FC.view_of("shares1", "real", dtype), q, dtype)
        bq = ref.bq.astype(FT[dtype]).astype(np.float64)             # the correctly rounded products pass
        ab = ref.abq.astype(FT[dtype]).astype(np.float64)
        assert max(ref.check(bq, ab)) <= 1.0
        j, i = int(np.argmax(ref.L)), int(np.argmax(ref.La))
        for bad_bq, bad_ab in ((bq + (np.arange(bv.rows) == j) * 300 * FC.UNIT[dtype] * float(ref.sbq[j]), ab),
                               (bq, ab + (np.arange(bv.m) == i) * 1200 * FC.UNIT[dtype] * float(ref.sab[i])),
                               (np.where(np.arange(bv.rows) == j, np.nan, bq), ab),                # a row nothing wrote
                               (bq + (np.arange(bv.rows) == int(np.argmin(ref.L))) * 1e-300, ab)):   # an empty row not 0
            with pytest.raises(AssertionError):
                ref.check(bad_bq, bad_ab)
        assert ref.L.min() == 0 and ref.L[j] <= 100 and ref.La[i] + ref.Lb[i] <= 400


# ---------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------
class _Pair:
    """The tiled operator of one case (values of `mode`, type `dtype`), its device transpose (of a shard: the
    rows lo:hi of it and their transpose), and device vectors; product() fills both outputs with NaN first."""

    def __init__(self, ctx, name, mode, dtype, shard=None):
        self.ctx, self.lib, self.dtype = ctx, L.load(), dtype
        c = FC.case(name)
        self.bv = FC.view_of(name, mode, dtype, shard)
        self.ops = []
        self.ft, self.es = FT[dtype], np.dtype(FT[dtype]).itemsize
        # NaN into blocks of the size of the operators' value arrays (4 values of padding behind nnz), freed
        # again: where the allocator hands such a block back, what the padding held is NaN, not zeros
        for _ in range(3):
            p = C.c_void_p()
            assert self.lib.hgm_dev_alloc(ctx.handle, self.es * (self.bv.nnz + 4), C.byref(p)) == L.HGM_OK
            self._put(p, np.full(self.bv.nnz + 4, np.nan))
            self.lib.hgm_dev_free(ctx.handle, p)
        A = hgmres.SparseOperator.from_scipy_tiled(c.matrix(mode, dtype), c.N, FC.TILE, 0, ctx=ctx, dtype=dtype)
        B = A.T
        self.ops += [A, B]
        if shard is not None:
            B = B.row_slice(*shard)
            A = B.T
            self.ops += [A, B]
        self.A, self.B = A, B
        self.pos = None if shard is not None else FC.stored_pixel_index(c.N)
        assert A.shape == (self.bv.m, self.bv.rows) and A.nnz == self.bv.nnz
        self.ptrs = [C.c_void_p() for _ in range(3)]
        for p, n in zip(self.ptrs, (self.bv.m, self.bv.rows, self.bv.m)):
            assert self.lib.hgm_dev_alloc(ctx.handle, self.es * max(1, n), C.byref(p)) == L.HGM_OK
        self.poison = None
        if shard is None:                               # (a tiled pair's Bq passes through a work buffer)
            n = c.N ** 2
            Sp = sp.csr_matrix((np.ones(n), np.arange(n, dtype=np.int32), np.array([0, n])), shape=(1, n))
            Ap = hgmres.SparseOperator.from_scipy_tiled(Sp, c.N, FC.TILE, 0, ctx=ctx, dtype=dtype)
            self.poison = (Ap, Ap.T)
            self.ops += list(self.poison)

    def _put(self, p, a):
        a = np.ascontiguousarray(a, dtype=self.ft)
        assert self.lib.hgm_memcpy_h2d(self.ctx.handle, p, a.ctypes.data_as(C.c_void_p), self.es * a.size) == L.HGM_OK

    def _get(self, p, n):
        out = np.empty(n, dtype=self.ft)
        assert self.lib.hgm_memcpy_d2h(self.ctx.handle, out.ctypes.data_as(C.c_void_p), p, self.es * n) == L.HGM_OK
        return out.astype(np.float64)

    def product(self, q):
        """(Bq in the stored row order of the view, A(Bq))"""
        qd, bqd, abd = self.ptrs
        m, n = self.bv.m, self.bv.rows
        if self.poison:                                 # NaN into every element of the work buffer
            with self.ctx.options(fused_ab=0):
                nan1 = hgmres.spmv_ab(self.poison[0], self.poison[1], np.array([np.nan]))
            assert np.all(np.isnan(nan1[0]))
        self._put(qd, q)
        self._put(bqd, np.full(n, np.nan))
        self._put(abd, np.full(m, np.nan))
        rc = self.lib.hgm_spmv_ab(self.ctx.handle, self.A._h, self.B._h, qd, bqd, abd)
        assert rc == L.HGM_OK, rc
        bq, ab = self._get(bqd, n), self._get(abd, m)
        if self.pos is not None:
            st = np.empty(n)
            st[self.pos] = bq
            bq = st
        return bq, ab

    def plan_info(self):
        """fused_plan_info, or None where the pair has no plan (the two-pass path)"""
        try:
            return hgmres.fused_plan_info(self.A, self.B)
        except ValueError as e:
            assert "this pair has none" in str(e), e
            return None

    def has_plan(self):
        return self.plan_info() is not None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            if p.value:
                self.lib.hgm_dev_free(self.ctx.handle, p)
        for o in self.ops:
            o.close()
        return False


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _report(capfd, monkeypatch, ctx, pair, **opts):
    """(plan info, the host plan build's own report) under the options, or (None, None) without a plan"""
    monkeypatch.setenv("HGM_FUSED_VERBOSE", "1")
    capfd.readouterr()
    try:
        with ctx.options(**opts):
            info = pair.plan_info()
        err = capfd.readouterr().err
    finally:
        monkeypatch.delenv("HGM_FUSED_VERBOSE")
    if info is None:
        return None, None
    mt = re.findall(r"\[fused rw plan\] region (\d+) waves (\d+) group (\d+):.*?max rays (\d+) \(LDS slots (\d+)\), "
                    r"longest row (\d+), (\d+) runs", err)
    assert mt, err
    rep = dict(zip(("region", "waves", "group", "worst", "slots", "maxlen", "runs"), (int(v) for v in mt[-1])))
    cd = re.findall(r"value stream\] (\d+) codes", err)
    rep["codes"] = int(cd[-1]) if cd else None
    return info, rep


# ---------------------------------------------------------------------------------------------
# GPU: the path taken
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name,shard", TARGETS, ids=TARGET_IDS)
def test_plan_is_the_twins(gpu_ctx, capfd, monkeypatch, name, shard, optset):
    """fused_plan_info and the host build's report against the twin: region, LDS slots, fullest region, runs,
    partial slots, compact or plain and the code count; the device build gives the same checksum."""
    dtype, opts, _ = OPTSETS[optset]
    p = _twin(name, optset, shard=shard)
    with _Pair(gpu_ctx, name, "real", dtype, shard) as pair:
        info, rep = _report(capfd, monkeypatch, gpu_ctx, pair, fused_ab=1, fused_plan_dev=0, **opts)
        if p["refused"]:
            assert info is None, (name, optset, p["refused"])
            with gpu_ctx.options(fused_ab=1, **opts):
                assert not pair.has_plan()
            return
        assert info is not None, (name, optset)
        print(f"PLAN {name} {optset}: {rep} nslot {info['nslot']} compact {info['vstream']}")
        assert (rep["region"], rep["waves"], rep["group"]) == (p["region"], 4, 8)
        assert (rep["slots"], rep["worst"], rep["maxlen"]) == (p["slots"], p["worst"], p["maxlen"])
        assert rep["runs"] == p["nruns"] and info["nslot"] == p["nslot"]
        assert info["vstream"] == p["compact"] and rep["codes"] == p["codes"]
        assert not info["device_built"]
        with gpu_ctx.options(fused_ab=1, fused_plan_dev=1, **opts):
            dev = hgmres.fused_plan_info(pair.A, pair.B)
        assert dev["device_built"] and dev["checksum"] == info["checksum"] and dev["vstream"] == info["vstream"]


# ---------------------------------------------------------------------------------------------
# GPU: exact inputs
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name,shard", TARGETS, ids=TARGET_IDS)
def test_exact_inputs_bit_for_bit(gpu_ctx, name, shard, optset):
    """values k/16, integer q: both products equal the integer result, whatever the summation order"""
    dtype, opts, _ = OPTSETS[optset]
    p = _twin(name, optset, "exact", shard)
    with _Pair(gpu_ctx, name, "exact", dtype, shard) as pair, gpu_ctx.options(fused_ab=1, **opts):
        assert pair.has_plan() == (not p["refused"])
        if not p["refused"]:
            assert hgmres.fused_plan_info(pair.A, pair.B)["vstream"] == p["compact"]
        bv = pair.bv
        inexact = FC.subnormal_rays(bv)[0]               # (their A(Bq) holds subnormal terms: the real-input check)
        keep = np.ones(bv.m, dtype=bool)
        keep[inexact] = False
        for label, q in FC.exact_qs(bv, dtype, _unit_rays(name, bv)):
            bq, ab, _, _ = FC.exact_products(bv, q)
            gbq, gab = pair.product(q)
            assert np.array_equal(gbq, bq), (name, optset, label, "Bq", np.flatnonzero(gbq != bq)[:8])
            assert np.all(np.isfinite(gab))
            assert np.array_equal(gab[keep], ab[keep]), (name, optset, label, "A(Bq)", np.flatnonzero(keep & (gab != ab))[:8])


# ---------------------------------------------------------------------------------------------
# GPU: real inputs
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name,shard", TARGETS, ids=TARGET_IDS)
def test_real_inputs_within_the_derived_bounds(gpu_ctx, name, shard, optset):
    """normal values and q against the np.longdouble sums: the gamma bounds of the module docstring"""
    dtype, opts, _ = OPTSETS[optset]
    p = _twin(name, optset, "real", shard)
    worst = [0.0, 0.0]
    with _Pair(gpu_ctx, name, "real", dtype, shard) as pair, gpu_ctx.options(fused_ab=1, **opts):
        assert pair.has_plan() == (not p["refused"])
        for seed in (1, 2):
            q = np.random.default_rng(seed).standard_normal(pair.bv.m)
            ref = FC.Reference(pair.bv, q, dtype)
            r = ref.check(*pair.product(q), what=(name, optset, seed))
            worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"RATIO {name} {optset}: largest |Bq - ref| / bound {worst[0]:.3f}, |A(Bq) - ref| / bound {worst[1]:.3f}")


# ---------------------------------------------------------------------------------------------
# GPU: equal bits wherever the code promises them
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("optset", list(OPTSETS))
@pytest.mark.parametrize("name,shard", TARGETS, ids=TARGET_IDS)
def test_equal_bits(gpu_ctx, name, shard, optset):
    dtype, opts, _ = OPTSETS[optset]
    p = _twin(name, optset, "real", shard)
    with _Pair(gpu_ctx, name, "real", dtype, shard) as pair:
        bv = pair.bv
        q = np.random.default_rng(5).standard_normal(bv.m)
        ref = FC.Reference(bv, q, dtype)
        with gpu_ctx.options(fused_ab=0):
            two = pair.product(q)
        ref.check(*two, what=(name, optset, "two-pass"))
        with gpu_ctx.options(fused_ab=1, **opts):
            assert pair.has_plan() == (not p["refused"])
            out = pair.product(q)
            ref.check(*out, what=(name, optset))
            assert _same(out, pair.product(q)), "a repeated call"
            if p["refused"]:
                assert _same(out, two), "a refused plan: the two-pass bits"
                return
            with gpu_ctx.options(fused_reduce=1):
                assert _same(out, pair.product(q)), "fused_reduce"
            for dev in (0, 1):
                with gpu_ctx.options(fused_plan_dev=dev):
                    assert hgmres.fused_plan_info(pair.A, pair.B)["device_built"] == bool(dev)
                    assert _same(out, pair.product(q)), ("fused_plan_dev", dev)
            if p["compact"]:
                for depth in (2, 3):
                    with gpu_ctx.options(fused_vsdepth=depth):
                        assert _same(out, pair.product(q)), ("fused_vsdepth", depth)
        if optset != "rp4vs3" or not p["compact"]:
            return
        # the decode is exact: compact (3, and 2: every value an escape) against plain on unit vectors
        hit = np.unique(bv.ci)
        rays = [int(hit[0]), int(hit[hit.size // 2]), int(hit[-1])] + [i for _, i in _unit_rays(name, bv)]
        for i in rays:
            e = np.zeros(bv.m)
            e[i] = 1.0
            with gpu_ctx.options(fused_ab=1, fused_rowpair=4, fused_vstream=0):
                assert not hgmres.fused_plan_info(pair.A, pair.B)["vstream"]
                plain = pair.product(e)
            FC.Reference(bv, e, dtype).check(*plain, what=(name, "unit", i))
            for vs in (3, 2):
                with gpu_ctx.options(fused_ab=1, fused_rowpair=4, fused_vstream=vs):
                    assert hgmres.fused_plan_info(pair.A, pair.B)["vstream"]
                    assert _same(plain, pair.product(e)), (name, "compact against plain", vs, i)


# ---------------------------------------------------------------------------------------------
# GPU: the one-pass Golub-Kahan step
# ---------------------------------------------------------------------------------------------
GK_CASES = ["len127", "len128", "len255", "len256", "shares1", "shares2"]
GK_STEPS = 3


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) /
                 max(np.linalg.norm(np.asarray(b, dtype=np.float64)), 1e-300))


@functools.lru_cache(maxsize=None)
def _gk_problem(name, dtype):
    S = FC.case(name).matrix("real", dtype)
    xt = np.random.default_rng(17).standard_normal(S.shape[1])
    return S, S @ xt, xt


@gpu
@pytest.mark.parametrize("dtype", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("solver", ["lsqr", "lsmr"])
@pytest.mark.parametrize("name", GK_CASES)
def test_golub_kahan_steps(gpu_ctx, name, solver, dtype):
    """Three iterations with fused_ab = 1 against fused_ab = 0 and the oracle: 1e-10 in fp64; in fp32
    max(1e-6, 100 x the fp32 oracle's spread over other summation orders (_Rounded32, 4 seeds))."""
    S, b, xt = _gk_problem(name, dtype)
    nh = 2 if solver == "lsqr" else 3
    gfn = {"lsqr": hgmres.lsqr_solver, "lsmr": hgmres.lsmr_solver}[solver]
    if dtype == 0:
        ofn = {"lsqr": R.lsqr_solver, "lsmr": R.lsmr_solver}[solver]
        ref = ofn(S, b, xt, 0.0, GK_STEPS)
        tx, th = 1e-10, [np.full(GK_STEPS, 1e-10)] * nh
    else:
        ofn = {"lsqr": R.lsqr_solver_f32, "lsmr": R.lsmr_solver_f32}[solver]
        A32 = sp.csr_matrix((S.data.astype(np.float32), S.indices, S.indptr), shape=S.shape)
        ref = ofn(A32, b, xt, 0.0, GK_STEPS)
        sx, sh = 0.0, [np.zeros(GK_STEPS) for _ in range(nh)]
        for seed in range(1, 5):
            o = ofn(_Rounded32(A32, np.random.default_rng(seed)), b, xt, 0.0, GK_STEPS)
            sx = max(sx, rel(o[0], ref[0]))
            for i in range(nh):
                sh[i] = np.maximum(sh[i], np.abs(o[1 + i] - ref[1 + i]) / np.abs(ref[1 + i]))
        tx, th = max(1e-6, 100.0 * sx), [np.maximum(1e-6, 100.0 * s) for s in sh]
    p = FC.plan_of(name, "real", dtype, 4, 1)
    with _Pair(gpu_ctx, name, "real", dtype) as pair:
        with gpu_ctx.options(fused_ab=0):
            two = gfn(pair.A, b, xt, 0.0, GK_STEPS, ctx=gpu_ctx, At=pair.B)
            assert gpu_ctx.solve_path()["one_pass"] == 0
        with gpu_ctx.options(fused_ab=1):
            assert pair.has_plan() == (not p["refused"])
            one = gfn(pair.A, b, xt, 0.0, GK_STEPS, ctx=gpu_ctx, At=pair.B)
            assert gpu_ctx.solve_path()["one_pass"] == (0 if p["refused"] else 1)
            again = gfn(pair.A, b, xt, 0.0, GK_STEPS, ctx=gpu_ctx, At=pair.B)
    assert one[-1] == two[-1] == ref[-1] == GK_STEPS
    assert all(np.array_equal(np.asarray(a), np.asarray(c)) for a, c in zip(one, again))
    devs = []
    for tag, other in (("two-pass", two), ("oracle", ref)):
        dx = rel(one[0], other[0])
        assert dx <= tx, (tag, "x", dx, tx)
        for i in range(nh):
            d = np.abs(np.asarray(one[1 + i]) - np.asarray(other[1 + i])) / np.abs(np.asarray(other[1 + i]))
            assert np.all(d <= th[i]), (tag, i, float(np.max(d / th[i])))
            dx = max(dx, float(np.max(d)))
        devs.append(f"{tag} {dx:.1e}")
    print(f"GK {name} {solver} {FT[dtype].__name__}: largest deviation " + ", ".join(devs) + f" (bar for x {tx:.1e})")
