// The matrix-free dense Gaussian perturbation (fp64, gfx950): G = randn(rows, cols) as a pure function
// of (seed, i, j), regenerated inside every product (hgm_gauss_*, and the E of hgm_spmm_pert_gauss /
// hgm_gmres_bounds_mismatch_gauss / hgm_arnoldi_mismatch_gauss).  Nothing of G is ever stored.
//
// Generator (hgmres/problems.py gaussian_entries is the host twin, step for step).  Indices are 0-based
// in the REFERENCE order.  For entry (i, j) with q = j >> 2, t = j & 3:
//   (w0..w3) = Philox4x32-10(counter (lo i, hi i, lo q, hi q), key (lo seed, hi seed));
//   pair p = t >> 1 takes (a, b) = (w[2p], w[2p+1]):  u = (a + 0.5) 2^-32 in (0, 1) exactly,
//   rad = sqrt(-2 log u) <= 6.77,  f = b 2^-31 in [0, 2) exactly;
//   g = rad * cospi(f) for even t, rad * sinpi(f) for odd t.
// One Philox call gives the four entries of a column quad; Box-Muller (not a rejection sampler) so every
// lane does the same bounded work and no loop depends on data.  -ffp-contract=off as the whole library.
//
//  * k_gauss_mm<NV, ACC>  Yi(i,r) = [Yi(i,r) +] (c_r * sum_j g(i,j) X(j,r)) on spmm.hip's interleaved
//        multi-vectors.  One wave works on GAUSS_R consecutive stored rows; lane l takes the quads
//        q = l, l + 64, ... in increasing order, loads the quad's 4*NV values of X ONCE (one contiguous
//        32*NV-byte piece) and uses them for all GAUSS_R rows, whose Philox calls and Box-Muller hide
//        the load.  Per (row, slot) the lane adds the quad's products in j order, each product rounded
//        and then added; the 64 lanes are combined by group_sum<64>.  So a slot's bits depend on the
//        reference row, cols, the seed, its own X column and its own c_r only: not on NV, the slot, the
//        other slots or coefficients, the grid, or the row tiling.
//        The counter takes the reference row: a stored row of a tiled pixel space is mapped through the
//        operator's row order (pixel_rc) once per row.  The columns are always in the reference order.
//  * k_gauss_entries      a block of entries, column-major (hgm_gauss_entries).
//  * k_gauss_rowsq / k_gauss_sum_rows   ||G||_F^2: per-row sums of squares in k_gauss_mm's lane order,
//        then the rows in a fixed order by one block; no atomics.
#include "device_common.h"

namespace hgm {

constexpr int GAUSS_R = 4;     // rows per wave that share one load of X

struct GaussCoef {
    double c[SPMM_MAXV];
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&w)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

// the four entries (i, 4q .. 4q+3)
__device__ __forceinline__ void gauss_quad(uint64_t seed, int64_t i, int64_t q, double (&g)[4]) {
    uint32_t w[4];
    philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)q, (uint32_t)((uint64_t)q >> 32),
                  (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const double u = ((double)w[2 * p] + 0.5) * 0x1p-32;
        const double rad = sqrt(-2.0 * log(u));
        const double f = (double)w[2 * p + 1] * 0x1p-31;
        double sn, cs;
        sincospi(f, &sn, &cs);
        g[2 * p] = rad * cs;
        g[2 * p + 1] = rad * sn;
    }
}

// reference row of stored row s (N == 0: the rows are in the reference order)
__device__ __forceinline__ int64_t gauss_ref_row(const PixOrder& o, int64_t s) {
    if (o.N == 0) return s;
    int64_t r, c;
    pixel_rc(o.N, o.tile, o.super, s, r, c);
    return r + c * o.N;
}

template <int NV, int ACC>
__global__ __launch_bounds__(BS) void k_gauss_mm(int64_t rows, int64_t cols, uint64_t seed, PixOrder ro,
                                                 GaussCoef cf, const double* __restrict__ Xi,
                                                 double* __restrict__ Yi) {
    constexpr int R = GAUSS_R;
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;                       // the whole wave: the butterflies stay inside a wave
    int64_t iref[R];
#pragma unroll
    for (int u = 0; u < R; ++u) iref[u] = row0 + u < rows ? gauss_ref_row(ro, row0 + u) : 0;
    double acc[R][NV];
#pragma unroll
    for (int u = 0; u < R; ++u)
#pragma unroll
        for (int r = 0; r < NV; ++r) acc[u][r] = 0.0;
    const int64_t nq = (cols + 3) >> 2;
    for (int64_t q = lane; q < nq; q += 64) {
        const int64_t left = cols - 4 * q;
        const int nt = left < 4 ? (int)left : 4;    // entries of this quad inside the matrix
        double x[4][NV];
        const double* p = Xi + 4 * q * NV;
        if (nt == 4) {
#pragma unroll
            for (int e = 0; e < 2 * NV; ++e) {      // 4*NV doubles, 32*NV-byte aligned
                const nd2 v = *reinterpret_cast<const nd2*>(p + 2 * e);
                x[(2 * e) / NV][(2 * e) % NV] = v.x;
                x[(2 * e + 1) / NV][(2 * e + 1) % NV] = v.y;
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < NV; ++r) x[t][r] = t < nt ? p[t * NV + r] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            if (row0 + u < rows) {                  // wave-uniform
                double g[4];
                gauss_quad(seed, iref[u], q, g);
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < NV; ++r) {
                        const double pr = g[t] * x[t][r];
                        const double s = acc[u][r] + pr;
                        acc[u][r] = t < nt ? s : acc[u][r];
                    }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
        double y[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) y[r] = cf.c[r] * group_sum<double, 64>(acc[u][r]);
        if (lane == u && row0 + u < rows) {
            double* yo = Yi + (row0 + u) * NV;
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                if constexpr (ACC) yo[r] = yo[r] + y[r];
                else yo[r] = y[r];
            }
        }
    }
}

// out[ii + ni * jj] = g(i0 + ii, j0 + jj)
__global__ __launch_bounds__(BS) void k_gauss_entries(uint64_t seed, int64_t i0, int64_t ni, int64_t j0, int64_t nj,
                                                      double* __restrict__ out) {
    const int64_t n = ni * nj;
    for (int64_t e = (int64_t)blockIdx.x * BS + threadIdx.x; e < n; e += (int64_t)gridDim.x * BS) {
        const int64_t ii = e % ni, j = j0 + e / ni;
        double g[4];
        gauss_quad(seed, i0 + ii, j >> 2, g);
        const int t = (int)(j & 3);
        out[e] = t == 0 ? g[0] : t == 1 ? g[1] : t == 2 ? g[2] : g[3];
    }
}

// rowsq[i] = sum_j g(i,j)^2: one wave per row, k_gauss_mm's lane order and butterfly
__global__ __launch_bounds__(BS) void k_gauss_rowsq(int64_t rows, int64_t cols, uint64_t seed,
                                                    double* __restrict__ rowsq) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (BS / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    double acc = 0.0;
    const int64_t nq = (cols + 3) >> 2;
    for (int64_t q = lane; q < nq; q += 64) {
        const int64_t left = cols - 4 * q;
        double g[4];
        gauss_quad(seed, row, q, g);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double pr = g[t] * g[t];
            const double s = acc + pr;
            acc = t < left ? s : acc;
        }
    }
    acc = group_sum<double, 64>(acc);
    if (lane == 0) rowsq[row] = acc;
}

// *out = sum_i rowsq[i]: thread t takes rows t, t + BS, ... in order, then the block sum (one block)
__global__ __launch_bounds__(BS) void k_gauss_sum_rows(int64_t rows, const double* __restrict__ rowsq,
                                                       double* __restrict__ out) {
    __shared__ double sh[BS / 64];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += BS) a += rowsq[i];
    const double s = block_sum_all<double, false>(a, sh);
    if (threadIdx.x == 0) out[0] = s;
}

static int64_t gauss_mm_blocks(int64_t rows) {
    const int64_t per = (int64_t)(BS / 64) * GAUSS_R;
    return (rows + per - 1) / per;
}

void gauss_mm(hgm_ctx* c, const hgm_gauss* G, const PixOrder& row_order, int nvec, const double* coefs, bool accumulate,
              const double* Xi, double* Yi) {
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "gauss_mm: 1 <= nvec <= 8");
    HGM_REQUIRE(row_order.trivial() || (int64_t)row_order.N * row_order.N == G->rows,
                "gauss_mm: the row order is not of G's rows");
    const int64_t nb = gauss_mm_blocks(G->rows);
    HGM_REQUIRE(nb <= 0x7fffffff, "gauss_mm: too many rows for one launch");
    GaussCoef cf;
    for (int r = 0; r < SPMM_MAXV; ++r) cf.c[r] = r < nvec ? (coefs ? coefs[r] : 1.0) : 0.0;
    const dim3 g((unsigned)nb), b(BS);
    dispatch(
        [&](auto nv, auto acc) {
            launch(c, false, k_gauss_mm<nv, acc>, g, b, G->rows, G->cols, G->seed, row_order, cf, Xi, Yi);
        },
        MvWidths{spmm_width(nvec)}, flag(accumulate));
    HGM_HIP(hipGetLastError());
}

void gauss_entries(hgm_ctx* c, const hgm_gauss* G, int64_t i0, int64_t ni, int64_t j0, int64_t nj, double* out_dev) {
    if (ni <= 0 || nj <= 0) return;
    hipLaunchKernelGGL(k_gauss_entries, dim3(grid_for(ni * nj)), dim3(BS), 0, c->stream, G->seed, i0, ni, j0, nj,
                       out_dev);
    HGM_HIP(hipGetLastError());
}

double gauss_fro(hgm_ctx* c, const hgm_gauss* G) {
    const int64_t nb = (G->rows + BS / 64 - 1) / (BS / 64);
    HGM_REQUIRE(nb <= 0x7fffffff, "gauss_fro: too many rows for one launch");
    double* rowsq = c->buf<double>("gauss_rowsq", (size_t)G->rows);
    double* out = c->buf<double>("gauss_fro", 1);
    hipLaunchKernelGGL(k_gauss_rowsq, dim3((unsigned)nb), dim3(BS), 0, c->stream, G->rows, G->cols, G->seed, rowsq);
    hipLaunchKernelGGL(k_gauss_sum_rows, dim3(1), dim3(BS), 0, c->stream, G->rows, (const double*)rowsq, out);
    HGM_HIP(hipGetLastError());
    double h = 0.0;
    Reader rd(c);
    rd.add(&h, out, sizeof(double));
    rd.go();
    return std::sqrt(h);
}

}  // namespace hgm
