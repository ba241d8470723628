// Block products on a Krylov / Lanczos basis (gfx950): the projections Q' X of several vectors at once
// and the rotated bases Q Y (Ritz / singular vectors), each in ONE pass over the basis (hgm_svds,
// the empirical filter factors of plot_filter_factors.m:30-40).
//
//   basis_project   C(j,r) = sum_i Q(i,j) X(i,r)     j < k <= 256, r < nx, groups of up to 8 columns of X
//   basis_rotate    W(i,l) = sum_j Q(i,j) Y(j,l)     l < p <= 64, W stored, optionally sum_i W(i,l)^2
//
// Both products run on the matrix cores (v_mfma_f64_16x16x4_f64), with the operand layouts of
// sweep.hip: A: lane l holds A[l & 15][l >> 4], B: lane l holds B[l >> 4][l & 15], C/D: lane l holds
// rows (l >> 4) + 4 r, r < 4, of column l & 15.
//
// basis_project.  The reduction runs over the rows, so the MFMA's K dimension is the row index: a
// wave takes tiles of 16 rows; for every block of 16 basis columns (up to 4 per workgroup, 64 columns,
// blockIdx.y) lane l loads Q[r0 + 4 t + (l >> 4)][j0 + (l & 15)], t < 4 (the A operand: M = basis
// column), and the B operand is X[r0 + 4 t + (l >> 4)][c0 + (l & 15)] (N = column of X, 8 of the 16
// used).  Every workgroup reads its own 64 columns of Q, so Q is read once per group of 8 columns of X,
// and X (8 columns) once per 64 columns of Q.  The 16 x 16 accumulators live in registers over all of
// a wave's tiles; then the four waves through LDS, the blocks through parts[(r k + j)][nb] and
// k_ba_finalize.
//
// basis_rotate.  The reduction runs over the basis columns: K = j, as in sweep.hip.  A wave owns tiles
// of 16 rows, loads the A operands Q[r0 + (l & 15)][4 q + (l >> 4)] once (whole 128-B lines) and
// multiplies them with the workgroup's chunk of Y staged in LDS (up to 4 column blocks; all p <= 64
// columns up to k = 92, else the chunks that fit 48 KiB, blockIdx.y): Q is read once per column chunk.
// Lane l stores W[r0 + (l >> 4) + 4 r][16 jb + (l & 15)] and adds its squares into the column's
// running sum.
//
// Every sum has a fixed order and there are no floating-point atomics: two calls give the same bits.
// The grid's row split depends on `rows` alone and a column's MFMA chain on its own data alone, so a
// column's bits do not depend on nx / p, on its position or on the other columns.  Rows >= rows,
// indices >= k, columns >= nx / p and padded leading dimensions are masked at the loads, never assumed
// zero (the masked operands are +0, which adds nothing to a sum).
#include <type_traits>

#include "device_common.h"

namespace hgm {

namespace {

typedef double nd4 __attribute__((ext_vector_type(4)));

constexpr int BP_G = 8;               // columns of X per pass of basis_project
constexpr int BP_JC = 64;             // basis columns per workgroup of basis_project (4 MFMA blocks)
constexpr int BA_KMAX = 256;          // basis columns of either kernel
constexpr int BR_PMAX = 64;           // columns of Y of basis_rotate (4 MFMA column blocks)
constexpr int BR_NJB = BR_PMAX / 16;
constexpr int BR_LDS_BYTES = 48 * 1024;
constexpr int BA_TILES_PER_WAVE = 4;  // at least this many row tiles per wave before the grid grows

// blocks along the rows: from the row count alone (the partial layout, so the bits, depend on it)
inline int ba_row_blocks(int64_t rows) {
    const int64_t ntiles = (rows + 15) / 16;
    int64_t nb = (ntiles + 4 * BA_TILES_PER_WAVE - 1) / (4 * BA_TILES_PER_WAVE);
    if (nb > MAX_PARTS) nb = MAX_PARTS;
    if (nb < 1) nb = 1;
    return (int)nb;
}

// NJB: blocks of 16 basis columns per workgroup (k <= 16 NJB, or 4 with blockIdx.y chunks of 64)
template <int NJB>
__global__ __launch_bounds__(BS) void k_basis_project(int64_t rows, int k, const double* __restrict__ Q, int64_t ldq,
                                                      int ng, const double* __restrict__ X, int64_t ldx,
                                                      double* __restrict__ parts) {
    __shared__ double red[4][NJB * 256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int j0 = blockIdx.y * (16 * NJB);
    const bool xok = lr < ng;
    const double* xp = X + (int64_t)(xok ? lr : 0) * ldx;
    nd4 acc[NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) acc[jb] = nd4{0.0, 0.0, 0.0, 0.0};

    const int64_t ntiles = (rows + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t r0 = (tile << 4) + lg;
        double xv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t i = r0 + 4 * t;
            xv[t] = (xok && i < rows) ? xp[i] : 0.0;
        }
        double qv[NJB][4];
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
            const int j = j0 + 16 * jb + lr;
            const bool jok = j < k;
            const double* qp = Q + (int64_t)(jok ? j : 0) * ldq;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int64_t i = r0 + 4 * t;
                qv[jb][t] = (jok && i < rows) ? qp[i] : 0.0;
            }
        }
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv[jb][t], xv[t], acc[jb], 0, 0, 0);
    }
    // the four waves (fixed order), then this block's partial of every (basis column, X column)
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][jb * 256 + r * 64 + lane] = acc[jb][r];
    __syncthreads();
    for (int e = threadIdx.x; e < NJB * 256; e += BS) {
        const int jb = e >> 8, r = (e >> 6) & 3, l = e & 63;
        const int j = j0 + 16 * jb + (l >> 4) + 4 * r, col = l & 15;
        if (j < k && col < ng) {
            const double v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
            parts[((int64_t)col * k + j) * gridDim.x + blockIdx.x] = v;
        }
    }
}

// block o: out[o] = sum of its nb partials
__global__ __launch_bounds__(BS) void k_ba_finalize(const double* __restrict__ parts, int nb, double* __restrict__ out) {
    __shared__ double sh[4];
    const int o = blockIdx.x;
    const double r = reduce_parts<double, false>(parts + (int64_t)o * nb, nb, sh);
    if (threadIdx.x == 0) out[o] = r;
}

// LDS stride of a staged Y column: odd, so the 16 columns a wave reads at once start in different banks
inline int br_lds_stride(int k) { return (((k + 3) / 4) * 4) | 1; }
// columns per workgroup (blockIdx.y chunks): a multiple of 16 that fits the LDS budget (all 64 up to k = 92)
inline int br_chunk_cols(int k, int p) {
    int lc = BR_LDS_BYTES / (br_lds_stride(k) * (int)sizeof(double)) / 16 * 16;
    if (lc > BR_PMAX) lc = BR_PMAX;
    const int p16 = (p + 15) / 16 * 16;
    return lc < p16 ? lc : p16;
}

// KQ > 0: the tile's A operands stay in KQ registers per lane (k <= 4 KQ); KQ == 0: any k, the
// operands are re-read (from cache) for every column block.  SUMS: also the columns' sums of squares.
template <int KQ, bool SUMS>
__global__ __launch_bounds__(BS) void k_basis_rotate(int64_t rows, int k, const double* __restrict__ Q, int64_t ldq,
                                                     const double* __restrict__ Y, int64_t ldy, int p, int lc,
                                                     double* __restrict__ W, int64_t ldw, double* __restrict__ parts) {
    extern __shared__ unsigned char br_smem[];
    double* ys = reinterpret_cast<double*>(br_smem);
    __shared__ double red[4][BR_PMAX];
    const int kq = (k + 3) >> 2;
    const int lds = (kq << 2) | 1;
    const int c0 = blockIdx.y * lc;                       // first column of this workgroup's chunk
    const int njb = lc >> 4;
    for (int e = threadIdx.x; e < lc * (kq << 2); e += BS) {
        const int col = e / (kq << 2), j = e - col * (kq << 2);
        ys[col * lds + j] = (j < k && c0 + col < p) ? Y[(int64_t)(c0 + col) * ldy + j] : 0.0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    double sacc[BR_NJB];
#pragma unroll
    for (int jb = 0; jb < BR_NJB; ++jb) sacc[jb] = 0.0;

    const int64_t ntiles = (rows + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t r0 = tile << 4;
        const bool rok = r0 + lr < rows;
        const double* qp = Q + r0 + lr;
        double a[KQ > 0 ? KQ : 1];
        if constexpr (KQ > 0) {
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int j = 4 * q + lg;
                a[q] = (rok && j < k) ? qp[(int64_t)j * ldq] : 0.0;
            }
        }
#pragma unroll
        for (int jb = 0; jb < BR_NJB; ++jb) {
            if (jb < njb) {
                const double* yp = ys + (jb * 16 + lr) * lds + lg;
                nd4 acc = {0.0, 0.0, 0.0, 0.0};
                if constexpr (KQ > 0) {
#pragma unroll
                    for (int q = 0; q < KQ; ++q)
                        if (q < kq) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q], yp[4 * q], acc, 0, 0, 0);
                } else {
                    for (int q = 0; q < kq; ++q) {
                        const int j = 4 * q + lg;
                        const double av = (rok && j < k) ? qp[(int64_t)j * ldq] : 0.0;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, yp[4 * q], acc, 0, 0, 0);
                    }
                }
                const int col = c0 + jb * 16 + lr;
                double* wp = W + (int64_t)(col < p ? col : 0) * ldw;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t i = r0 + lg + 4 * r;
                    const double w = acc[r];
                    if (col < p && i < rows) wp[i] = w;
                    if constexpr (SUMS) {
                        // rows >= rows hold exact zeros (masked A operands): they add nothing
                        const double ww = w * w;
                        sacc[jb] += ww;
                    }
                }
            }
        }
    }
    if constexpr (SUMS) {
        // the four lane groups of a column, then the four waves, then this block's partial
#pragma unroll
        for (int jb = 0; jb < BR_NJB; ++jb) {
            double s = sacc[jb];
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (lg == 0) red[wave][jb * 16 + lr] = s;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < lc; e += BS)
            if (c0 + e < p)
                parts[(int64_t)(c0 + e) * gridDim.x + blockIdx.x] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
    }
}

}  // namespace

void basis_project(hgm_ctx* c, int64_t rows, int k, const double* Q, int64_t ldq, int nx, const double* X, int64_t ldx,
                   double* C_dev) {
    HGM_REQUIRE(rows >= 1 && k >= 1 && nx >= 1, "basis_project: rows, k and the column count must be >= 1");
    HGM_REQUIRE(k <= BA_KMAX, "basis_project: k must be <= 256");
    HGM_REQUIRE(ldq >= rows && ldx >= rows, "basis_project: leading dimensions shorter than the columns");
    HGM_REQUIRE(Q != nullptr && X != nullptr && C_dev != nullptr, "basis_project: Q, X and the output are required");
    const int nb = ba_row_blocks(rows);
    double* parts = c->buf<double>("bp_parts", (size_t)BP_G * k * nb);
    hipEvent_t tm;
    timing_begin(c, KC_BASIS, &tm);
    for (int c0 = 0; c0 < nx; c0 += BP_G) {
        const int ng = nx - c0 < BP_G ? nx - c0 : BP_G;
        const double* Xg = X + (int64_t)c0 * ldx;
        // 16-column MFMA blocks of the basis per workgroup: the fewest that hold k, BP_JC / 16 at most
        using ProjectBlocks = Ints<1, 2, BP_JC / 16>;
        dispatch(
            [&](auto njb) {
                const dim3 grid((unsigned)nb, (unsigned)((k + 16 * njb - 1) / (16 * njb)));
                k_basis_project<njb><<<grid, BS, 0, c->stream>>>(rows, k, Q, ldq, ng, Xg, ldx, parts);
            },
            ProjectBlocks{k <= 16 ? 1 : k <= 32 ? 2 : BP_JC / 16});
        k_ba_finalize<<<ng * k, BS, 0, c->stream>>>(parts, nb, C_dev + (size_t)c0 * k);
    }
    HGM_HIP(hipGetLastError());
    const double groups = (double)((nx + BP_G - 1) / BP_G);
    timing_end(c, KC_BASIS, tm, 8.0 * (double)rows * (groups * k + (double)nx * ((k + BP_JC - 1) / BP_JC)));
}

void basis_rotate(hgm_ctx* c, int64_t rows, int k, const double* Q, int64_t ldq, int p, const double* Y, int64_t ldy,
                  double* W, int64_t ldw, double* sumsq_dev) {
    HGM_REQUIRE(rows >= 1 && k >= 1 && p >= 1, "basis_rotate: rows, k and the column count must be >= 1");
    HGM_REQUIRE(k <= BA_KMAX, "basis_rotate: k must be <= 256");
    HGM_REQUIRE(p <= BR_PMAX, "basis_rotate: at most 64 columns");
    HGM_REQUIRE(ldq >= rows && ldy >= k && ldw >= rows, "basis_rotate: leading dimensions shorter than the columns");
    HGM_REQUIRE(Q != nullptr && Y != nullptr && W != nullptr, "basis_rotate: Q, Y and W are required");
    const int nb = ba_row_blocks(rows);
    double* parts = sumsq_dev ? c->buf<double>("br_parts", (size_t)BR_PMAX * nb) : nullptr;
    const int lc = br_chunk_cols(k, p);
    const dim3 grid((unsigned)nb, (unsigned)((p + lc - 1) / lc));
    const size_t lds = sizeof(double) * (size_t)lc * br_lds_stride(k);
    hipEvent_t tm;
    timing_begin(c, KC_BASIS, &tm);
    // KQ of the kernel: the smallest instantiated register count with k <= 4 KQ, else 0 (operands re-read)
    using RotateSteps = Ints<1, 2, 4, 8, 16, 24, 0>;
    const int kq = k <= 4 ? 1 : k <= 8 ? 2 : k <= 16 ? 4 : k <= 32 ? 8 : k <= 64 ? 16 : k <= 96 ? 24 : 0;
    dispatch(
        [&](auto kqv, auto sums) {
            constexpr bool S = sums;
            k_basis_rotate<kqv, S><<<grid, BS, lds, c->stream>>>(rows, k, Q, ldq, Y, ldy, p, lc, W, ldw, parts);
        },
        RotateSteps{kq}, flag(sumsq_dev != nullptr));
    if (sumsq_dev) k_ba_finalize<<<p, BS, 0, c->stream>>>(parts, nb, sumsq_dev);
    HGM_HIP(hipGetLastError());
    timing_end(c, KC_BASIS, tm, 8.0 * (double)rows * ((double)k * grid.y + p));
}

}  // namespace hgm
