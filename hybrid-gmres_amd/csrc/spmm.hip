// Multi-vector sparse products (fp64, gfx950): Y(:,r) = M X(:,r) for up to 8 vectors with ONE pass
// over the operator's entries (hgm_spmm, and the operator of hgm_gmres_bounds_batch).
//
// Layout: an interleaved multi-vector of width NV in {1, 2, 4, 8} stores element (i, r) at
// Xi[i*NV + r], so the NV values an entry (val, col) multiplies are one contiguous 8*NV-byte
// gather.  The streaming SpMVs make about one L1 tag lookup per entry and are bound by that
// address path, not by HBM (spmv.hip, "Paged x gathers"); here the lookup, the 12 B/entry operator
// stream and the address arithmetic are paid once per entry for all NV vectors.
//
//  * k_spmm<NV, G>  one G-lane group per CSR row (G = hgm_mat::group: pick_group, from the operator
//                   alone).  Lane gl takes entries s+gl, s+gl+G, ... in that order, U of them in
//                   flight (all index/value loads, then all gathers, then the FMAs), one register
//                   accumulator per vector; a fixed butterfly over the G lanes; lane 0 stores the
//                   row's NV results contiguously.  No atomics, no LDS, no scratch.
//  * k_pack / k_unpack  between up to NV column-major vectors (a pointer table) and the interleaved
//                   form; unused slots are written as zeros.
//
// Invariance: slot r's accumulator sees v_0 x_0, v_1 x_1, ... of its lane's entries in entry order
// whatever NV is and whatever the other slots hold (the unroll depth only changes how many loads are
// in flight), and the butterfly is group_sum<G>.  So a column's bits depend on the row and G only:
// not on the vector count, its slot, or its neighbours.  The batch solver relies on this.
#include "device_common.h"

namespace hgm {

template <int NV>
__device__ __forceinline__ void mv_gather(const double* __restrict__ Xi, int32_t col, double (&x)[NV]) {
    const double* p = Xi + (int64_t)col * NV;
    if constexpr (NV == 1) {
        x[0] = p[0];
    } else {
#pragma unroll
        for (int t = 0; t < NV / 2; ++t) {
            const nd2 v = *reinterpret_cast<const nd2*>(p + 2 * t);
            x[2 * t] = v.x;
            x[2 * t + 1] = v.y;
        }
    }
}

template <int NV, int G>
__global__ __launch_bounds__(BS) void k_spmm(int64_t rows, const int64_t* __restrict__ rp,
                                             const int32_t* __restrict__ ci, const double* __restrict__ val,
                                             const double* __restrict__ Xi, double* __restrict__ Yi) {
    constexpr int RPB = BS / G;
    constexpr int U = 4;   // entries per lane in flight
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / G;
    const int gl = threadIdx.x & (G - 1);
    double acc[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = 0.0;
    if (row < rows) {
        const int64_t e = rp[row + 1];
        int64_t i = rp[row] + gl;
        for (; i + (U - 1) * G < e; i += U * G) {
            int32_t cc[U];
            double vv[U];
            double xx[U][NV];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cc[u] = ld<true>(ci + i + u * G);
                vv[u] = ld<true>(val + i + u * G);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) mv_gather<NV>(Xi, cc[u], xx[u]);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int r = 0; r < NV; ++r) acc[r] = __builtin_fma(vv[u], xx[u][r], acc[r]);
        }
        for (; i < e; i += G) {
            const int32_t cc = ld<true>(ci + i);
            const double vv = ld<true>(val + i);
            double xx[NV];
            mv_gather<NV>(Xi, cc, xx);
#pragma unroll
            for (int r = 0; r < NV; ++r) acc[r] = __builtin_fma(vv, xx[r], acc[r]);
        }
    }
    // every lane of the block takes part in the butterfly (rows past the end carry zeros)
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = group_sum<double, G>(acc[r]);
    if (gl == 0 && row < rows) {
        double* y = Yi + row * NV;
        if constexpr (NV == 1) {
            y[0] = acc[0];
        } else {
#pragma unroll
            for (int t = 0; t < NV / 2; ++t) {
                nd2 v;
                v.x = acc[2 * t];
                v.y = acc[2 * t + 1];
                *reinterpret_cast<nd2*>(y + 2 * t) = v;
            }
        }
    }
}

// Xi[i*NV + r] = src.p[r][i] for r < nv, 0 for the unused slots.  Thread i reads element i of every
// column (coalesced per column) and writes its NV values contiguously.
template <int NV>
__global__ __launch_bounds__(BS) void k_pack(int64_t n, int nv, MvCols src, double* __restrict__ Xi) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double v[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) v[r] = r < nv ? src.p[r][i] : 0.0;
        double* x = Xi + i * NV;
        if constexpr (NV == 1) {
            x[0] = v[0];
        } else {
#pragma unroll
            for (int t = 0; t < NV / 2; ++t) {
                nd2 w;
                w.x = v[2 * t];
                w.y = v[2 * t + 1];
                *reinterpret_cast<nd2*>(x + 2 * t) = w;
            }
        }
    }
}

// dst.p[r][i] = Yi[i*NV + r] for r < nv
template <int NV>
__global__ __launch_bounds__(BS) void k_unpack(int64_t n, int nv, const double* __restrict__ Yi, MvCols dst) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double v[NV];
        const double* y = Yi + i * NV;
        if constexpr (NV == 1) {
            v[0] = y[0];
        } else {
#pragma unroll
            for (int t = 0; t < NV / 2; ++t) {
                const nd2 w = *reinterpret_cast<const nd2*>(y + 2 * t);
                v[2 * t] = w.x;
                v[2 * t + 1] = w.y;
            }
        }
#pragma unroll
        for (int r = 0; r < NV; ++r)
            if (r < nv) dst.p[r][i] = v[r];
    }
}

int spmm_width(int nvec) { return nvec <= 1 ? 1 : nvec <= 2 ? 2 : nvec <= 4 ? 4 : 8; }

// blocks of a grid-stride elementwise pass over n rows of an interleaved multi-vector
static int mv_grid(int64_t n) {
    int64_t nb = (n + BS - 1) / BS;
    if (nb > 16384) nb = 16384;
    return (int)(nb < 1 ? 1 : nb);
}

void mv_pack(hgm_ctx* c, int64_t n, int nvec, const MvCols& src, double* Xi) {
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "mv_pack: 1 <= nvec <= 8");
    if (n <= 0) return;
    const dim3 g(mv_grid(n)), b(BS);
    switch (spmm_width(nvec)) {
        case 1: launch(c, false, k_pack<1>, g, b, n, nvec, src, Xi); break;
        case 2: launch(c, false, k_pack<2>, g, b, n, nvec, src, Xi); break;
        case 4: launch(c, false, k_pack<4>, g, b, n, nvec, src, Xi); break;
        default: launch(c, false, k_pack<8>, g, b, n, nvec, src, Xi); break;
    }
    HGM_HIP(hipGetLastError());
}

void mv_unpack(hgm_ctx* c, int64_t n, int nvec, const double* Yi, const MvCols& dst, bool last) {
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "mv_unpack: 1 <= nvec <= 8");
    if (n <= 0) return;
    const dim3 g(mv_grid(n)), b(BS);
    switch (spmm_width(nvec)) {
        case 1: launch(c, last, k_unpack<1>, g, b, n, nvec, Yi, dst); break;
        case 2: launch(c, last, k_unpack<2>, g, b, n, nvec, Yi, dst); break;
        case 4: launch(c, last, k_unpack<4>, g, b, n, nvec, Yi, dst); break;
        default: launch(c, last, k_unpack<8>, g, b, n, nvec, Yi, dst); break;
    }
    HGM_HIP(hipGetLastError());
}

template <int NV>
static void launch_spmm(hgm_ctx* c, const hgm_mat* M, const double* Xi, double* Yi) {
    const double* val = reinterpret_cast<const double*>(M->val);
#define HGM_SPMM_G(GV)                                                                                         \
    {                                                                                                          \
        const int64_t nb = (M->rows + (BS / GV) - 1) / (BS / GV);                                              \
        HGM_REQUIRE(nb <= 0x7fffffff, "spmm: too many rows for one launch");                                   \
        launch(c, false, k_spmm<NV, GV>, dim3((unsigned)nb), dim3(BS), M->rows, M->rp, M->ci, val, Xi, Yi);    \
    }
    switch (M->group) {
        case 64: HGM_SPMM_G(64) break;
        case 32: HGM_SPMM_G(32) break;
        case 16: HGM_SPMM_G(16) break;
        case 8: HGM_SPMM_G(8) break;
        default: HGM_SPMM_G(4) break;
    }
#undef HGM_SPMM_G
}

void spmm(hgm_ctx* c, const hgm_mat* M, int nvec, const double* Xi, double* Yi) {
    HGM_REQUIRE(M->dtype == HGM_F64, "spmm: fp64 operators only");
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "spmm: 1 <= nvec <= 8");
    HGM_REQUIRE(M->cols <= 0x7fffffff, "spmm: 32-bit column indices");
    if (M->rows <= 0) return;
    switch (spmm_width(nvec)) {
        case 1: launch_spmm<1>(c, M, Xi, Yi); break;
        case 2: launch_spmm<2>(c, M, Xi, Yi); break;
        case 4: launch_spmm<4>(c, M, Xi, Yi); break;
        default: launch_spmm<8>(c, M, Xi, Yi); break;
    }
    HGM_HIP(hipGetLastError());
}

}  // namespace hgm
