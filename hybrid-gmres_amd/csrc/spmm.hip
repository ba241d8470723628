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
//  * k_spmm_pert<NV, G, SHARED>  the same walk for Y(:,r) = B0 X(:,r) + c_r E X(:,r) with per-slot
//                   coefficients (hgm_spmm_pert, the B pass of hgm_gmres_bounds_mismatch); see below.
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
    dispatch([&](auto nv) { launch(c, false, k_pack<nv>, g, b, n, nvec, src, Xi); }, MvWidths{spmm_width(nvec)});
    HGM_HIP(hipGetLastError());
}

void mv_unpack(hgm_ctx* c, int64_t n, int nvec, const double* Yi, const MvCols& dst, bool last) {
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "mv_unpack: 1 <= nvec <= 8");
    if (n <= 0) return;
    const dim3 g(mv_grid(n)), b(BS);
    dispatch([&](auto nv) { launch(c, last, k_unpack<nv>, g, b, n, nvec, Yi, dst); }, MvWidths{spmm_width(nvec)});
    HGM_HIP(hipGetLastError());
}

void spmm(hgm_ctx* c, const hgm_mat* M, int nvec, const double* Xi, double* Yi) {
    HGM_REQUIRE(M->dtype == HGM_F64, "spmm: fp64 operators only");
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "spmm: 1 <= nvec <= 8");
    HGM_REQUIRE(M->cols <= 0x7fffffff, "spmm: 32-bit column indices");
    if (M->rows <= 0) return;
    const double* val = reinterpret_cast<const double*>(M->val);
    dispatch(
        [&](auto nv, auto g) {
            const int64_t nb = (M->rows + (BS / g) - 1) / (BS / g);
            HGM_REQUIRE(nb <= 0x7fffffff, "spmm: too many rows for one launch");
            launch(c, false, k_spmm<nv, g>, dim3((unsigned)nb), dim3(BS), M->rows, M->rp, M->ci, val, Xi, Yi);
        },
        MvWidths{spmm_width(nvec)}, RowGroups{M->group});
    HGM_HIP(hipGetLastError());
}

// ============================================================================
// Perturbed multi-vector product: Y(i,r) = (B0 X)(i,r) + c_r (E X)(i,r)
// ============================================================================
// The operator of the mismatch sweep (hgm_gmres_bounds_mismatch): slot r applies B0 + c_r E, and no
// such operator is ever formed.  One G-lane group per row with G = B0->group, k_spmm's lane / entry
// assignment, load batching and butterfly, and two accumulators per slot: accB sees B0's entries and
// accE sees E's, each in its lane's entry order, so accB is k_spmm's accumulator on B0 bit for bit and
// accE is k_spmm<NV, G>'s on E.  The coefficients enter only the last line, y = accB + (c_r * accE):
// two roundings, no contraction (EPI_ADD's convention), so slot r's bits depend on the row, G and c_r
// only -- not on NV, the slot, the other slots or their coefficients.
//  * SHARED = 1: E has B0's rp / ci (decided on the device, same_pattern).  One index load and one
//    gather per entry serve both value streams: 20 B/entry instead of 24, half the gathers.
//  * SHARED = 0: E has a pattern of its own; the group walks B0's row, then E's.
// Both sum accE over the same entries in the same order, so for a same-pattern E they agree bit for bit.
// U (entries per lane in flight) does not affect bits.  NV = 8 holds 16 accumulators (32 VGPRs) and
// 16 U registers of gathered doubles: with U = 2 the compiler reports 70 VGPRs for the shared path and
// 84 for the general one (7 and 5 waves per SIMD, no scratch); U = 4 would add 32 and drop both to 4
// waves for two more entries in flight per lane.  The narrower widths have room for k_spmm's U = 4.
struct PertCoef {
    double c[SPMM_MAXV];
};

template <int NV>
constexpr int pert_unroll() { return NV == 8 ? 2 : 4; }

// acc[r] += sum over this lane's entries of row [i0 - gl, e) of val * X(col, r), in entry order
template <int NV, int G, int U>
__device__ __forceinline__ void pert_row(const int32_t* __restrict__ ci, const double* __restrict__ val, int64_t i,
                                         int64_t e, const double* __restrict__ Xi, double (&acc)[NV]) {
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

template <int NV, int G, int SHARED>
__global__ __launch_bounds__(BS) void k_spmm_pert(int64_t rows, const int64_t* __restrict__ rpB,
                                                  const int32_t* __restrict__ ciB, const double* __restrict__ valB,
                                                  const int64_t* __restrict__ rpE, const int32_t* __restrict__ ciE,
                                                  const double* __restrict__ valE, PertCoef cf,
                                                  const double* __restrict__ Xi, double* __restrict__ Yi) {
    constexpr int RPB = BS / G;
    constexpr int U = pert_unroll<NV>();
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / G;
    const int gl = threadIdx.x & (G - 1);
    double accB[NV], accE[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) accB[r] = accE[r] = 0.0;
    if (row < rows) {
        if constexpr (SHARED) {
            const int64_t e = rpB[row + 1];
            int64_t i = rpB[row] + gl;
            for (; i + (U - 1) * G < e; i += U * G) {
                int32_t cc[U];
                double vb[U], ve[U];
                double xx[U][NV];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    cc[u] = ld<true>(ciB + i + u * G);
                    vb[u] = ld<true>(valB + i + u * G);
                    ve[u] = ld<true>(valE + i + u * G);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) mv_gather<NV>(Xi, cc[u], xx[u]);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int r = 0; r < NV; ++r) {
                        accB[r] = __builtin_fma(vb[u], xx[u][r], accB[r]);
                        accE[r] = __builtin_fma(ve[u], xx[u][r], accE[r]);
                    }
            }
            for (; i < e; i += G) {
                const int32_t cc = ld<true>(ciB + i);
                const double vb = ld<true>(valB + i);
                const double ve = ld<true>(valE + i);
                double xx[NV];
                mv_gather<NV>(Xi, cc, xx);
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    accB[r] = __builtin_fma(vb, xx[r], accB[r]);
                    accE[r] = __builtin_fma(ve, xx[r], accE[r]);
                }
            }
        } else {
            pert_row<NV, G, U>(ciB, valB, rpB[row] + gl, rpB[row + 1], Xi, accB);
            pert_row<NV, G, U>(ciE, valE, rpE[row] + gl, rpE[row + 1], Xi, accE);
        }
    }
    // every lane of the block takes part in the butterflies (rows past the end carry zeros)
    double y[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) {
        const double b = group_sum<double, G>(accB[r]);
        const double s = cf.c[r] * group_sum<double, G>(accE[r]);
        y[r] = b + s;
    }
    if (gl == 0 && row < rows) {
        double* yo = Yi + row * NV;
        if constexpr (NV == 1) {
            yo[0] = y[0];
        } else {
#pragma unroll
            for (int t = 0; t < NV / 2; ++t) {
                nd2 v;
                v.x = y[2 * t];
                v.y = y[2 * t + 1];
                *reinterpret_cast<nd2*>(yo + 2 * t) = v;
            }
        }
    }
}

// *differ = 1 when the two CSR index streams differ anywhere (rows + 1 row pointers, nnz columns)
__global__ __launch_bounds__(BS) void k_pattern_differs(int64_t rows, int64_t nnz, const int64_t* __restrict__ rpA,
                                                        const int64_t* __restrict__ rpB,
                                                        const int32_t* __restrict__ ciA,
                                                        const int32_t* __restrict__ ciB, double* differ) {
    bool d = false;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i <= rows; i += (int64_t)gridDim.x * BS)
        d |= rpA[i] != rpB[i];
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * BS)
        d |= ciA[i] != ciB[i];
    if (d) *differ = 1.0;
}

bool same_pattern(hgm_ctx* c, const hgm_mat* B0, const hgm_mat* E) {
    if (B0->rows != E->rows || B0->cols != E->cols || B0->nnz != E->nnz) return false;
    if (B0->rp == E->rp && B0->ci == E->ci) return true;
    double* differ = c->buf<double>("pert_differ", 1);
    HGM_HIP(hipMemsetAsync(differ, 0, sizeof(double), c->stream));
    const int64_t len = std::max<int64_t>(B0->rows + 1, B0->nnz);
    hipLaunchKernelGGL(k_pattern_differs, dim3(mv_grid(len)), dim3(BS), 0, c->stream, B0->rows, B0->nnz, B0->rp,
                       E->rp, B0->ci, E->ci, differ);
    HGM_HIP(hipGetLastError());
    double h = 1.0;
    Reader rd(c);
    rd.add(&h, differ, sizeof(double));
    rd.go();
    return h == 0.0;
}

void spmm_pert(hgm_ctx* c, const hgm_mat* B0, const hgm_mat* E, bool shared, int nvec, const double* coefs,
               const double* Xi, double* Yi) {
    HGM_REQUIRE(B0->dtype == HGM_F64 && E->dtype == HGM_F64, "spmm_pert: fp64 operators only");
    HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "spmm_pert: 1 <= nvec <= 8");
    HGM_REQUIRE(B0->rows == E->rows && B0->cols == E->cols, "spmm_pert: E must have B0's shape");
    HGM_REQUIRE(B0->cols <= 0x7fffffff, "spmm_pert: 32-bit column indices");
    HGM_REQUIRE(!shared || B0->nnz == E->nnz, "spmm_pert: the shared path needs E on B0's pattern");
    if (B0->rows <= 0) return;
    PertCoef cf;
    for (int r = 0; r < SPMM_MAXV; ++r) cf.c[r] = r < nvec ? coefs[r] : 0.0;
    const double* vb = reinterpret_cast<const double*>(B0->val);
    const double* ve = reinterpret_cast<const double*>(E->val);
    dispatch(
        [&](auto nv, auto sh, auto g) {
            const int64_t nb = (B0->rows + (BS / g) - 1) / (BS / g);
            HGM_REQUIRE(nb <= 0x7fffffff, "spmm_pert: too many rows for one launch");
            launch(c, false, k_spmm_pert<nv, g, sh>, dim3((unsigned)nb), dim3(BS), B0->rows, B0->rp, B0->ci, vb, E->rp,
                   E->ci, ve, cf, Xi, Yi);
        },
        MvWidths{spmm_width(nvec)}, flag(shared), RowGroups{B0->group});
    HGM_HIP(hipGetLastError());
}

}  // namespace hgm
