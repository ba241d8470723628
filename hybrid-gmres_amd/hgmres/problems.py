"""Synthetic 2-D parallel-beam tomography problems (the input side of the hot path).

The reference's only 2-D case comes from the un-vendored ``PRtomo_mismatched``
(``run_2D_phantom.m:12-15``) and its ``generate_test_problem.m:1-11`` only
dispatches to 1-D Regularization-Tools problems, so the operators for the
BASELINE configs are built here:

* ``A``  – ray-driven Siddon line-integral projector, CSR, one row per ray
  (ray-major), ``m = p * n_angles`` rows with ``p = ceil(sqrt(2) N)``
  detectors of unit spacing; ``n = N*N`` pixels of unit size, pixel index in
  MATLAB column-major order ``col*N + row``.
* ``B``  – the back-projector: ``A^T`` (matched, pixel-major CSR) or an
  unmatched pixel-driven linear-interpolation back-projector (the classic
  ray-driven/pixel-driven mismatched pair the reference studies).
* ``x_true`` – modified Shepp–Logan phantom, ``b = A x_true + e`` with
  ``||e|| = eta ||A x_true||`` (as ``run_2D_phantom.m:18-20``).

Detector positions are offset by a quarter spacing so no ray runs exactly
along a pixel boundary (keeps pixel assignment well defined for every
implementation of the generator).

This module is host (numpy) code: it produces the operands that the C-ABI
library uploads; it is not part of the timed path.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

DETECTOR_OFFSET = 0.25

# BASELINE.json configs -> (N, n_angles)   (SURVEY.md §8(d) "Synthetic inputs")
CONFIGS = {
    "c1": (64, 90),      # 64^2, m=8,190,  nnz~4.7e5 (CPU plumbing case)
    "c2": (512, 30),     # 512^2, m=21,750, nnz~1.0e7 (hybrid_ab_gmres_rtp, 1 GPU)
    "c3": (2048, 19),    # 2048^2, m=55,043, nnz~1.0e8 (BA-GMRES + GCV, MGS vs CGS2)
    "c4": (4096, 47),    # 4096^2, m=272,271, nnz~1.0e9 (AB-GMRES, 8 GPUs)
}


def geometry(N: int, n_angles: int):
    """Parallel-beam geometry: detector count, angles, detector offsets."""
    p = int(math.ceil(math.sqrt(2.0) * N))
    theta = np.arange(n_angles, dtype=np.float64) * (np.pi / n_angles)
    s = np.arange(p, dtype=np.float64) - (p - 1) / 2.0 + DETECTOR_OFFSET
    return p, theta, s


def _siddon_chunk(N, cos_t, sin_t, s):
    """Siddon ray tracing for a chunk of parallel rays (direction (cos_t, sin_t), signed
    detector offset s from the centre).  Returns (counts, cols, vals) with the entries of each
    ray ordered along the ray (increasing t)."""
    return _siddon_rays(N, -s * sin_t, s * cos_t, cos_t, sin_t)


def _siddon_rays(N, x0, y0, cos_t, sin_t):
    """Siddon ray tracing for a chunk of rays x(t) = (x0, y0) + t (cos_t, sin_t) (unit direction)
    over the N x N grid of unit pixels centred on the origin.  Returns (counts, cols, vals)
    with the entries of each ray ordered along the ray (increasing t).  Mirrored by the device
    generators' ray_geom / siddon_walk (csrc/ops.hip)."""
    half = N / 2.0
    grid = np.arange(N + 1, dtype=np.float64) - half
    eps = 1e-12
    cx = np.abs(cos_t) > eps
    cy = np.abs(sin_t) > eps
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = (grid[None, :] - x0[:, None]) / np.where(cx, cos_t, 1.0)[:, None]
        ty = (grid[None, :] - y0[:, None]) / np.where(cy, sin_t, 1.0)[:, None]
    inf = np.inf
    txmin = np.where(cx, np.minimum(tx[:, 0], tx[:, N]), np.where(np.abs(x0) < half, -inf, inf))
    txmax = np.where(cx, np.maximum(tx[:, 0], tx[:, N]), np.where(np.abs(x0) < half, inf, -inf))
    tymin = np.where(cy, np.minimum(ty[:, 0], ty[:, N]), np.where(np.abs(y0) < half, -inf, inf))
    tymax = np.where(cy, np.maximum(ty[:, 0], ty[:, N]), np.where(np.abs(y0) < half, inf, -inf))
    tmin = np.maximum(txmin, tymin)
    tmax = np.minimum(txmax, tymax)
    hit = tmin < tmax
    tx = np.where(cx[:, None], tx, inf)
    ty = np.where(cy[:, None], ty, inf)
    T = np.concatenate([tx, ty, tmin[:, None], tmax[:, None]], axis=1)
    lo = tmin[:, None]
    hi = tmax[:, None]
    T = np.where((T >= lo) & (T <= hi) & hit[:, None], T, inf)
    T.sort(axis=1)
    t0 = T[:, :-1]
    t1 = T[:, 1:]
    with np.errstate(invalid="ignore"):
        L = t1 - t0
    valid = np.isfinite(t1) & (L > 1e-10)
    mid = 0.5 * (t0 + t1)
    with np.errstate(invalid="ignore"):
        xm = x0[:, None] + mid * cos_t[:, None]
        ym = y0[:, None] + mid * sin_t[:, None]
    ix = np.clip(np.floor(np.where(valid, xm, 0.0) + half), 0, N - 1).astype(np.int64)
    iy = np.clip(np.floor(np.where(valid, ym, 0.0) + half), 0, N - 1).astype(np.int64)
    col = ix * N + (N - 1 - iy)          # column-major pixel index, row 0 = top
    counts = valid.sum(axis=1)
    return counts, col[valid].astype(np.int32), L[valid]


def siddon_projector(N: int, n_angles: int, chunk_elems: int = 1 << 24) -> sp.csr_matrix:
    """Ray-major CSR of the parallel-beam line-integral operator (m x N^2).
    Entries of each row are in along-ray order (increasing t), exactly as the
    device generator ``hgm_mat_create_siddon`` emits them."""
    p, theta, s = geometry(N, n_angles)
    # C-libm cos/sin (math module), identical to the device generator's host-side geometry
    cos_t = np.array([math.cos(t) for t in theta])
    sin_t = np.array([math.sin(t) for t in theta])
    m = p * n_angles
    rays_per_chunk = max(1, chunk_elems // (2 * N + 4))
    counts_all, cols_all, vals_all = [], [], []
    ray = 0
    while ray < m:
        r1 = min(m, ray + rays_per_chunk)
        idx = np.arange(ray, r1)
        a = idx // p
        d = idx % p
        cnt, col, val = _siddon_chunk(N, cos_t[a], sin_t[a], s[d])
        counts_all.append(cnt)
        cols_all.append(col)
        vals_all.append(val)
        ray = r1
    counts = np.concatenate(counts_all)
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    A = sp.csr_matrix((np.concatenate(vals_all), np.concatenate(cols_all), indptr), shape=(m, N * N))
    A.has_sorted_indices = False
    return A


FAN_R = 2.0          # source-to-centre distance in units of N (this repository's choice; see fan_geometry)


def _fan_tables(N, n_angles, R, span, det_offset):
    """(p, D, cb, sb, co, so) of the fan geometry: the C-libm cos / sin of the source angles
    beta_a and of the fan angles omega_d, as the device generators' host side forms them."""
    p = int(math.ceil(math.sqrt(2.0) * N))
    if span is None:
        span = 2.0 * math.asin(1.0 / (math.sqrt(2.0) * R))
    D = R * N
    dom = span / p
    cb = np.array([math.cos(a * (2.0 * math.pi / n_angles)) for a in range(n_angles)])
    sb = np.array([math.sin(a * (2.0 * math.pi / n_angles)) for a in range(n_angles)])
    om = [((d - (p - 1) / 2.0) + det_offset) * dom for d in range(p)]
    co = np.array([math.cos(w) for w in om])
    so = np.array([math.sin(w) for w in om])
    return p, D, cb, sb, co, so


def fan_geometry(N: int, n_angles: int, R: float = FAN_R, span: float | None = None,
                 det_offset: float = DETECTOR_OFFSET):
    """Fan-beam, curved (equiangular) detector geometry standing in for the CTtype 'fancurved' of
    run_2D_phantom.m:12-13.  PRtomo_mismatched is not vendored by the reference and no fixture of
    it exists, so this geometry is the repository's OWN choice, modelled on a curved-detector fan
    beam; parity with PRtomo_mismatched / AIR Tools II fanbeamtomo is UNPINNED.  Its
    departures from fanbeamtomo as commonly documented (unverifiable offline): p = ceil(sqrt(2) N)
    rays per source (fanbeamtomo reportedly rounds), a fan span fitted to the circumscribed circle
    rather than a user angle, and source angles equispaced over a full turn.  The geometry:
    * source angles beta_a = a * 2 pi / n_angles (a full turn), the source at distance D = R N
      from the centre, S_a = D (cos beta_a, sin beta_a);
    * p = ceil(sqrt(2) N) rays per source position at fan angles
      omega_d = ((d - (p-1)/2) + det_offset) * span / p, d = 0..p-1 (equiangular bins: a curved
      detector on an arc around the source);
    * span (radians) defaults to the fan that just covers the image's circumscribed circle,
      2 asin(1 / (sqrt(2) R));
    * ray (a, d) leaves S_a towards the centre rotated by omega_d: direction
      u = -(cos(beta + omega), sin(beta + omega)), formed by the angle-addition formula from the
      C-libm cos / sin of beta and omega (the same IEEE operations on the host and the device).
    Row index a * p + d (source-angle-major, as the parallel geometry).  Returns
    (p, x0, y0, ux, uy) per ray."""
    p, D, cb, sb, co, so = _fan_tables(N, n_angles, R, span, det_offset)
    cbr, sbr = np.repeat(cb, p), np.repeat(sb, p)
    cor, sor = np.tile(co, n_angles), np.tile(so, n_angles)
    x0 = D * cbr
    y0 = D * sbr
    ux = -(cbr * cor - sbr * sor)
    uy = -(sbr * cor + cbr * sor)
    return p, x0, y0, ux, uy


def fanbeam_projector(N: int, n_angles: int, R: float = FAN_R, span: float | None = None,
                      det_offset: float = DETECTOR_OFFSET, chunk_elems: int = 1 << 24) -> sp.csr_matrix:
    """Ray-major CSR of the fan-beam (curved detector) line-integral operator (fan_geometry),
    entries of each row in along-ray order; bit-identical to the device generator
    ``hgm_mat_create_fanbeam``."""
    p, x0, y0, ux, uy = fan_geometry(N, n_angles, R, span, det_offset)
    m = p * n_angles
    rays_per_chunk = max(1, chunk_elems // (2 * N + 4))
    counts_all, cols_all, vals_all = [], [], []
    for r0 in range(0, m, rays_per_chunk):
        sl = slice(r0, min(m, r0 + rays_per_chunk))
        cnt, col, val = _siddon_rays(N, x0[sl], y0[sl], ux[sl], uy[sl])
        counts_all.append(cnt)
        cols_all.append(col)
        vals_all.append(val)
    counts = np.concatenate(counts_all)
    indptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    A = sp.csr_matrix((np.concatenate(vals_all), np.concatenate(cols_all), indptr), shape=(m, N * N))
    A.has_sorted_indices = False
    return A


def pixel_driven_backprojector(N: int, n_angles: int) -> sp.csr_matrix:
    """Unmatched back-projector B (n x m, pixel-major CSR): for every pixel
    centre and angle, linear interpolation between the two nearest detector
    bins.  Weights per (pixel, angle) sum to 1, the scale of A^T."""
    p, theta, s = geometry(N, n_angles)
    half = N / 2.0
    n = N * N
    pix = np.arange(n, dtype=np.int64)
    c = pix // N
    r = pix % N
    xc = c - half + 0.5
    yc = (N - 1 - r) - half + 0.5
    rows, cols, vals = [], [], []
    for a in range(n_angles):
        sa = -xc * math.sin(float(theta[a])) + yc * math.cos(float(theta[a]))
        df = sa + (p - 1) / 2.0 - DETECTOR_OFFSET
        d0 = np.floor(df).astype(np.int64)
        w1 = df - d0
        for dd, w in ((d0, 1.0 - w1), (d0 + 1, w1)):
            ok = (dd >= 0) & (dd < p) & (w > 0)
            rows.append(pix[ok])
            cols.append((a * p + dd[ok]).astype(np.int64))
            vals.append(w[ok])
    rows = np.concatenate(rows)
    cols = np.concatenate(cols)
    vals = np.concatenate(vals)
    B = sp.csr_matrix((vals, (rows, cols)), shape=(n, p * n_angles))
    B.sum_duplicates()
    B.sort_indices()
    return B


def fan_pixel_sides(N: int, pix, cb, sb, D: float):
    """(along, across), each len(pix) x n_angles, of the pixel centres ``pix`` (reference index
    c*N + r) seen from every source of the fan geometry: with v = centre - source,
    along = -(v . (cb, sb)) and across = sb vx - cb vy, so that ray d passes the centre on the side
    s(d) = across * co[d] - along * so[d] = |v| sin(gamma - omega_d).  Every product and sum is
    rounded on its own, in the order of the device kernel (csrc/ops.hip k_fan_backproj)."""
    half = N / 2.0
    pix = np.asarray(pix, dtype=np.int64)
    xc = ((pix // N) - half) + 0.5
    yc = ((N - 1 - pix % N) - half) + 0.5
    vx = xc[:, None] - (D * cb)[None, :]
    vy = yc[:, None] - (D * sb)[None, :]
    along = -(vx * cb[None, :] + vy * sb[None, :])
    across = sb[None, :] * vx - cb[None, :] * vy
    return along, across


def fan_pixel_backprojector(N: int, n_angles: int, R: float = FAN_R, span: float | None = None,
                            det_offset: float = DETECTOR_OFFSET, chunk_elems: int = 1 << 20) -> sp.csr_matrix:
    """Unmatched back-projector B (n x m, pixel-major CSR) of the fan-beam geometry
    (:func:`fan_geometry`, same arguments), pairing with :func:`fanbeam_projector`: for every
    pixel centre and source, linear interpolation in the fan angle between the two rays that
    bracket the centre.  With s(d) of :func:`fan_pixel_sides`, d0 is the result of the bisection
    lo = -1, hi = p; mid = (lo + hi) >> 1; lo = mid if s(mid) >= 0 else hi = mid; a centre outside
    the fan [omega_0, omega_{p-1}) (d0 < 0 or d0 >= p - 1) gets nothing from that source, the
    others w1 = s(d0) / (s(d0) - s(d0+1)) at column a*p + d0 + 1 and w0 = 1 - w1 at a*p + d0
    (where positive), so the weights per (pixel, source) sum to 1: no distance weighting.  This is
    the repository's own stand-in for PRtomo_mismatched with CTtype 'fancurved'
    (run_2D_phantom.m:12-15); parity with it is UNPINNED.  Bit-identical to the device generator
    ``hgm_mat_create_fan_backprojector``.  Chunked over pixels: the largest temporaries are
    chunk x n_angles."""
    p, D, cb, sb, co, so = _fan_tables(N, n_angles, R, span, det_offset)
    n = N * N
    chunk = max(1, chunk_elems // n_angles)
    col0 = (np.arange(n_angles, dtype=np.int64) * p)[None, :]
    counts_all, cols_all, vals_all = [], [], []
    for p0 in range(0, n, chunk):
        along, across = fan_pixel_sides(N, np.arange(p0, min(n, p0 + chunk)), cb, sb, D)

        def side(d):
            return across * co[d] - along * so[d]

        lo = np.full(along.shape, -1, dtype=np.int64)
        hi = np.full(along.shape, p, dtype=np.int64)
        while True:
            act = hi - lo > 1
            if not act.any():
                break
            mid = np.where(act, (lo + hi) >> 1, 0)
            ge = side(mid) >= 0
            lo = np.where(act & ge, mid, lo)
            hi = np.where(act & ~ge, mid, hi)
        ok = (lo >= 0) & (lo < p - 1)
        d0 = np.where(ok, lo, 0)
        s0, s1 = side(d0), side(d0 + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            w1 = s0 / (s0 - s1)
        w0 = 1.0 - w1
        keep = np.stack([ok & (w0 > 0), ok & (w1 > 0)], axis=2)
        cols = np.stack([col0 + d0, col0 + d0 + 1], axis=2)
        vals = np.stack([w0, w1], axis=2)
        counts_all.append(keep.sum(axis=(1, 2)))
        cols_all.append(cols[keep].astype(np.int32))
        vals_all.append(vals[keep])
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.concatenate(counts_all), out=indptr[1:])
    return sp.csr_matrix((np.concatenate(vals_all), np.concatenate(cols_all), indptr), shape=(n, p * n_angles))


# ---------------------------------------------------------------------------
# The matrix-free dense Gaussian perturbation (csrc/gauss.hip): entry (i, j) of randn(size(A')) as a
# pure function of (seed, i, j).  This is the host twin of the device generator, step for step.
# ---------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
GAUSS_ENTRIES_MAX = 1 << 27


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), vectorised: counter words ``c0..c3`` and key words ``k0, k1``
    are uint64 arrays (or scalars) holding 32-bit values; returns the four output words as uint64 arrays."""
    m32 = np.uint64(0xffffffff)
    sh = np.uint64(32)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & m32
                                                   for v in (c0, c1, c2, c3, k0, k1)])
    M0, M1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    W0, W1 = np.uint64(PHILOX_W0), np.uint64(PHILOX_W1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & m32, (p0 >> sh) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + W0) & m32, (k1 + W1) & m32
    return c0, c1, c2, c3


def gaussian_entries(rows, cols, seed, i0=0, ni=None, j0=0, nj=None):
    """The ``ni x nj`` block at (i0, j0) of the ``rows x cols`` standard normal matrix of ``seed`` (64 bits),
    0-based in the reference order.  Entry (i, j) depends on (seed, i, j) alone: one Philox4x32-10 call with
    counter (i, j >> 2) gives the four entries of a column quad by Box-Muller, all in fp64:
    ``u = (a + 0.5) 2^-32``, ``rad = sqrt(-2 log u)``, ``f = b 2^-31``, ``rad cospi(f)`` for even ``j``
    and ``rad sinpi(f)`` for odd ``j``, with (a, b) words (0, 1) of the call for ``j & 3 < 2``, else (2, 3).
    ``cospi`` / ``sinpi`` reduce ``f`` exactly to the nearest multiple of 1/2, so every factor has relative
    error only."""
    rows, cols, seed = int(rows), int(cols), int(seed) & 0xffffffffffffffff
    ni = rows - i0 if ni is None else int(ni)
    nj = cols - j0 if nj is None else int(nj)
    if rows < 1 or cols < 1:
        raise ValueError("gaussian_entries: rows, cols >= 1")
    if i0 < 0 or j0 < 0 or ni < 0 or nj < 0 or i0 + ni > rows or j0 + nj > cols:
        raise ValueError(f"gaussian_entries: block ({i0}:{i0 + ni}, {j0}:{j0 + nj}) outside {rows} x {cols}")
    out = np.empty((ni, nj))
    if ni == 0 or nj == 0:
        return out
    q0, q1 = j0 >> 2, (j0 + nj - 1) >> 2
    i = (np.arange(ni, dtype=np.uint64) + np.uint64(i0))[:, None]
    q = (np.arange(q1 - q0 + 1, dtype=np.uint64) + np.uint64(q0))[None, :]
    sh = np.uint64(32)
    w = philox4x32_10(i, i >> sh, q, q >> sh, np.uint64(seed & 0xffffffff), np.uint64(seed >> 32))
    quad = np.empty((ni, q1 - q0 + 1, 4))
    for p in range(2):
        a, b = w[2 * p], w[2 * p + 1].astype(np.int64)
        u = (a.astype(np.float64) + 0.5) * 2.0 ** -32
        rad = np.sqrt(-2.0 * np.log(u))
        k = (b + (1 << 29)) >> 30                      # nearest multiple of 1/2 to f = b 2^-31
        r = (b - (k << 30)).astype(np.float64) * 2.0 ** -31     # exact, in [-1/4, 1/4]
        cr, sr = np.cos(np.pi * r), np.sin(np.pi * r)
        k &= 3
        cosv = np.where(k == 0, cr, np.where(k == 1, -sr, np.where(k == 2, -cr, sr)))
        sinv = np.where(k == 0, sr, np.where(k == 1, cr, np.where(k == 2, -sr, -cr)))
        quad[:, :, 2 * p] = rad * cosv
        quad[:, :, 2 * p + 1] = rad * sinv
    lo = j0 - 4 * q0
    out[:] = quad.reshape(ni, -1)[:, lo:lo + nj]
    return out


def shepp_logan(N: int) -> np.ndarray:
    """Modified (Toft) Shepp–Logan phantom on an N x N grid, values in [0, 1].
    Row 0 is the top of the image (y = +1)."""
    E = [  # intensity, a, b, x0, y0, phi(deg)
        (1.0, 0.69, 0.92, 0.0, 0.0, 0.0),
        (-0.8, 0.6624, 0.8740, 0.0, -0.0184, 0.0),
        (-0.2, 0.1100, 0.3100, 0.22, 0.0, -18.0),
        (-0.2, 0.1600, 0.4100, -0.22, 0.0, 18.0),
        (0.1, 0.2100, 0.2500, 0.0, 0.35, 0.0),
        (0.1, 0.0460, 0.0460, 0.0, 0.1, 0.0),
        (0.1, 0.0460, 0.0460, 0.0, -0.1, 0.0),
        (0.1, 0.0460, 0.0230, -0.08, -0.605, 0.0),
        (0.1, 0.0230, 0.0230, 0.0, -0.606, 0.0),
        (0.1, 0.0230, 0.0460, 0.06, -0.605, 0.0),
    ]
    g = (np.arange(N) + 0.5) / N * 2.0 - 1.0
    X, Y = np.meshgrid(g, -g)          # Y[0, :] = top row
    P = np.zeros((N, N))
    for I, a, b, x0, y0, phi in E:
        ph = math.radians(phi)
        xr = (X - x0) * math.cos(ph) + (Y - y0) * math.sin(ph)
        yr = -(X - x0) * math.sin(ph) + (Y - y0) * math.cos(ph)
        P[(xr / a) ** 2 + (yr / b) ** 2 <= 1.0] += I
    return np.clip(P, 0.0, 1.0)


@dataclass
class TomoProblem:
    N: int
    n_angles: int
    p: int
    A: sp.csr_matrix          # m x n, ray-major
    B: sp.csr_matrix          # n x m, pixel-major back-projector
    b: np.ndarray             # noisy sinogram (m)
    b_exact: np.ndarray
    x_true: np.ndarray        # phantom, column-major (n)

    @property
    def m(self):
        return self.A.shape[0]

    @property
    def n(self):
        return self.A.shape[1]


def tomo_problem(N: int, n_angles: int, noise: float = 1e-2, seed: int = 0,
                 backprojector: str = "matched", geometry_kind: str = "parallel") -> TomoProblem:
    """Build (A, B, b, x_true).  ``backprojector`` is ``"matched"`` (B = A^T),
    ``"pixel"`` (unmatched pixel-driven B, parallel beam only) or ``"fanpixel"`` (unmatched
    pixel-driven B of the fan beam, :func:`fan_pixel_backprojector`, fan beam only).
    ``geometry_kind``: ``"parallel"`` (Siddon, angles over [0, pi)) or ``"fan"`` (curved-detector
    fan beam over a full turn, :func:`fan_geometry`)."""
    if geometry_kind == "fan":
        if backprojector not in ("matched", "fanpixel"):
            raise ValueError("the fan-beam geometry pairs with the 'matched' or the 'fanpixel' back-projector")
        A = fanbeam_projector(N, n_angles)
    elif geometry_kind == "parallel":
        if backprojector == "fanpixel":
            raise ValueError("the 'fanpixel' back-projector pairs with the fan-beam geometry only")
        A = siddon_projector(N, n_angles)
    else:
        raise ValueError("geometry_kind must be 'parallel' or 'fan'")
    p = geometry(N, n_angles)[0]
    x_true = shepp_logan(N).ravel(order="F")
    b_exact = A @ x_true
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(A.shape[0])
    e = e / np.linalg.norm(e) * noise * np.linalg.norm(b_exact)
    b = b_exact + e
    if backprojector == "matched":
        B = A.T.tocsr()
        B.sort_indices()
    elif backprojector == "pixel":
        B = pixel_driven_backprojector(N, n_angles)
    elif backprojector == "fanpixel":
        B = fan_pixel_backprojector(N, n_angles)
    else:
        raise ValueError("backprojector must be 'matched', 'pixel' or 'fanpixel'")
    return TomoProblem(N, n_angles, p, A, B, b, b_exact, x_true)


def config_problem(name: str, **kw) -> TomoProblem:
    N, na = CONFIGS[name]
    return tomo_problem(N, na, **kw)
