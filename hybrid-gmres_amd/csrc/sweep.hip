// Multi-coefficient projected norms for the lambda sweep of the hybrid PTR solvers (gfx950).
//
// For V (rows x k, column-major, leading dimension ldv), Y (k x L, column-major) and an optional
// vector t (rows), every column l gets
//     d_l = sum_i (sum_j V_ij Y_jl - t_i)^2        s_l = sum_i (sum_j V_ij Y_jl)^2
// in ONE pass over V: the rows x L product is a tall-skinny GEMM whose result is squared and summed
// in the epilogue and never stored.  2kL flops per 8k bytes of V = L/4 flop/B, so from a few tens
// of columns on the pass is bound by the fp64 issue rate, not by HBM: the products run on the
// matrix cores (v_mfma_f64_16x16x4_f64).  (basis.hip's block kernels are the library's
// other fp64 MFMA use.)
//
// Layout.  A wave owns tiles of 16 rows.  Per tile it loads the MFMA A operands once, one double per
// lane and k-quad: lane l holds V[16 tile + (l & 15)][4 q + (l >> 4)] (16 consecutive rows of one
// column per lane group: whole 128-B lines), k zero-padded to a multiple of 4.  The workgroup's
// chunk of Y (up to PN_LC columns, blockIdx.y) sits in LDS, zero-padded in both directions, and is
// the B operand: lane l reads Y[4 q + (l >> 4)][16 jb + (l & 15)].  In the f64 C/D layout lane l
// then holds rows (l >> 4) + 4 r, r < 4, of column 16 jb + (l & 15): it subtracts its four t_i,
// squares and adds into its two running sums of that column.  Reduction, all in fixed order (no
// floating-point atomics, so two runs give the same bits): the four lane groups by xor shuffles,
// the four waves through LDS, the blocks through parts[2 L][nb] and k_pn_finalize.
// Rows >= rows, k-indices >= k and columns >= L are masked at the loads, never assumed zero.
#include <type_traits>

#include "device_common.h"

namespace hgm {

namespace {

typedef double nd4 __attribute__((ext_vector_type(4)));

constexpr int PN_LC = 128;            // columns of Y per workgroup (8 MFMA column blocks)
constexpr int PN_NJB = PN_LC / 16;
constexpr int PN_KMAX = 256;          // 16 columns of Y of this height still fit the LDS budget
constexpr int PN_LDS_BYTES = 48 * 1024;
constexpr int PN_TILES_PER_WAVE = 4;  // at least this many row tiles per wave before the grid grows

// LDS stride of a staged Y column: odd, so the 16 columns a wave reads at once start in
// different banks
inline int pn_lds_stride(int k) { return (((k + 3) / 4) * 4) | 1; }
// columns per workgroup: a multiple of 16 that fits the LDS budget
inline int pn_chunk_cols(int k, int L) {
    int lc = PN_LDS_BYTES / (pn_lds_stride(k) * (int)sizeof(double)) / 16 * 16;
    if (lc > PN_LC) lc = PN_LC;
    const int l16 = (L + 15) / 16 * 16;
    return lc < l16 ? lc : l16;
}

// KQ > 0: the tile's A operands stay in KQ registers per lane (k <= 4 KQ); KQ == 0: any k, the
// operands are re-read (from cache) for every column block.
template <int KQ>
__global__ __launch_bounds__(BS) void k_proj_norms(int64_t rows, int k, const double* __restrict__ V, int64_t ldv,
                                                   const double* __restrict__ Y, int64_t ldy, int L, int lc,
                                                   const double* __restrict__ t, double* __restrict__ parts) {
    extern __shared__ unsigned char pn_smem[];
    double* ys = reinterpret_cast<double*>(pn_smem);
    __shared__ double red[4][2 * PN_LC];
    const int kq = (k + 3) >> 2;
    const int lds = (kq << 2) | 1;
    const int c0 = blockIdx.y * lc;                       // first column of this workgroup's chunk
    const int njb = lc >> 4;
    for (int e = threadIdx.x; e < lc * (kq << 2); e += BS) {
        const int col = e / (kq << 2), j = e - col * (kq << 2);
        ys[col * lds + j] = (j < k && c0 + col < L) ? Y[(int64_t)(c0 + col) * ldy + j] : 0.0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    double dacc[PN_NJB], sacc[PN_NJB];
#pragma unroll
    for (int jb = 0; jb < PN_NJB; ++jb) dacc[jb] = sacc[jb] = 0.0;

    const int64_t ntiles = (rows + 15) >> 4;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t r0 = tile << 4;
        const bool rok = r0 + lr < rows;
        const double* vp = V + r0 + lr;
        double a[KQ > 0 ? KQ : 1];
        if constexpr (KQ > 0) {
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                const int j = 4 * q + lg;
                a[q] = (rok && j < k) ? vp[(int64_t)j * ldv] : 0.0;
            }
        }
        double tv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = r0 + lg + 4 * r;
            tv[r] = (t != nullptr && i < rows) ? t[i] : 0.0;
        }
#pragma unroll
        for (int jb = 0; jb < PN_NJB; ++jb) {
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
                        const double av = (rok && j < k) ? vp[(int64_t)j * ldv] : 0.0;
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, yp[4 * q], acc, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double p = acc[r];
                    const double d = p - tv[r];
                    const double pp = p * p, dd = d * d;
                    sacc[jb] += pp;
                    dacc[jb] += dd;
                }
            }
        }
    }
    // the four lane groups of a column, then the four waves, then this block's partial
#pragma unroll
    for (int jb = 0; jb < PN_NJB; ++jb) {
        double d = dacc[jb], s = sacc[jb];
        d += __shfl_xor(d, 16);
        s += __shfl_xor(s, 16);
        d += __shfl_xor(d, 32);
        s += __shfl_xor(s, 32);
        if (lg == 0) {
            red[wave][jb * 16 + lr] = d;
            red[wave][PN_LC + jb * 16 + lr] = s;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * PN_LC; e += BS) {
        const int which = e / PN_LC, col = e - which * PN_LC;
        if (col < lc && c0 + col < L) {
            const double v = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
            parts[((int64_t)which * L + c0 + col) * gridDim.x + blockIdx.x] = v;
        }
    }
}

// block o < L: d_out[o] = sum of its nb partials; block L + o: s_out[o]
__global__ __launch_bounds__(BS) void k_pn_finalize(const double* __restrict__ parts, int nb, int L,
                                                    double* __restrict__ d_out, double* __restrict__ s_out) {
    __shared__ double sh[4];
    const int o = blockIdx.x;
    const double r = reduce_parts<double, false>(parts + (int64_t)o * nb, nb, sh);
    if (threadIdx.x == 0) {
        if (o < L) d_out[o] = r;
        else s_out[o - L] = r;
    }
}

}  // namespace

template <typename T>
void proj_norms(hgm_ctx* c, int64_t rows, int k, const T* V, int64_t ldv, const T* Y, int64_t ldy, int L,
                const T* t, T* d_out, T* s_out) {
    static_assert(std::is_same<T, double>::value, "proj_norms is fp64");
    HGM_REQUIRE(rows >= 1 && k >= 1 && L >= 1, "proj_norms: rows, k and the column count must be >= 1");
    HGM_REQUIRE(k <= PN_KMAX, "proj_norms: k must be <= 256");
    HGM_REQUIRE(ldv >= rows && ldy >= k, "proj_norms: leading dimensions shorter than the columns");
    HGM_REQUIRE(V != nullptr && Y != nullptr && d_out != nullptr, "proj_norms: V, Y and the output are required");
    const int lc = pn_chunk_cols(k, L);
    const int nchunks = (L + lc - 1) / lc;
    const int64_t ntiles = (rows + 15) / 16;
    int64_t nb = (ntiles + 4 * PN_TILES_PER_WAVE - 1) / (4 * PN_TILES_PER_WAVE);
    if (nb > MAX_PARTS) nb = MAX_PARTS;
    if (nb < 1) nb = 1;
    double* parts = c->buf<double>("pn_parts", (size_t)2 * L * nb);
    const size_t lds = sizeof(double) * (size_t)lc * pn_lds_stride(k);
    const dim3 grid((unsigned)nb, (unsigned)nchunks);
    // KQ of the kernel: the smallest instantiated register count with k <= 4 KQ, else 0 (operands re-read)
    using ProjSteps = Ints<1, 2, 4, 8, 16, 0>;
    const int kq = k <= 4 ? 1 : k <= 8 ? 2 : k <= 16 ? 4 : k <= 32 ? 8 : k <= 64 ? 16 : 0;
    dispatch([&](auto kqv) { k_proj_norms<kqv><<<grid, BS, lds, c->stream>>>(rows, k, V, ldv, Y, ldy, L, lc, t, parts); },
             ProjSteps{kq});
    k_pn_finalize<<<s_out ? 2 * L : L, BS, 0, c->stream>>>(parts, (int)nb, L, d_out, s_out);
    HGM_HIP(hipGetLastError());
}

template void proj_norms<double>(hgm_ctx*, int64_t, int, const double*, int64_t, const double*, int64_t, int,
                                 const double*, double*, double*);

}  // namespace hgm
