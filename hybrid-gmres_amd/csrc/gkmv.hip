// Golub-Kahan recurrences on interleaved multi-vectors (fp64, gfx950): the vector kernels of the
// lockstep LSQR / LSMR solves (hgm_gk_batch) and of hgm_mv_axpby_norms.
//
// Layout: spmm.hip's.  An interleaved multi-vector of width NV in {1, 2, 4, 8} stores element (i, r)
// at X[i*NV + r], so spmm(A) / spmm(At) run on the solver's state with no pack or unpack in between.
// Per-slot coefficients travel by value (MvCoef, 8 doubles, as PertCoef).
//
//  * k_mv_lin<NV, NT>   Out(i,r) = (a_r X(i,r)) [+ (b_r Y(i,r)) [+ (c_r Z(i,r))]]: every product is
//                       rounded, then the sums left to right (-ffp-contract=off: no FMA; EPI_ADD /
//                       EPI_SUB's convention).  a = 1 is exact and b = -alpha negates exactly, so
//                       (1*t) + (-alpha*u) is the reference's A*v - alpha*u bit for bit.  Optional
//                       per-slot sums: sum Out^2, or sum (Out - D)^2 with D interleaved or one vector
//                       shared by every slot.  Out == nullptr: the sums alone.  Out may alias an input.
//  * k_mv_div<NV>       Out = In / s_r, a true division (div_scalar); guard: left as it is unless
//                       s_r > 0 (lsmr_solver.m:12 / :16 / :36 / :40).
//  * k_mv_lsqr_step<NV> lsqr_solver.m:28, :40-41 in one launch: v = v_hat / alpha, x = x + (c_x w),
//                       w = v - (c_w w), with the terms of ||x - x_true||^2 (:43).
//  * k_mv_lsmr_step<NV> lsmr_solver.m:40, :61-67 in one launch: v = v_hat / alpha (alpha > 0), the
//                       hbar / x / h updates, with the terms of ||x - x_true||^2 (:72).
//  * k_mv_regather<NV>  new slot r = slot src[r] of an old group of any width (columns leaving a batch).
//
// Every kernel gives thread g of the grid rows g, g + G, ... (G = the grid's threads) and all NV slots
// of a row: NV >= 2 moves a row as 16-byte pairs.  The grid depends on the vector length only
// (gkmv_grid).  Sums: each lane adds its rows' terms in row order, then wave_sum, then the block's four
// waves through LDS in block_sum_all's order, then parts[slot][block], then k_mv_finalize (reduce_parts,
// k_finalize's order) -- no atomics.  A slot's lane sees the same rows whatever NV is, so a slot's
// elements and sums depend on its own data and the length only: not on NV, the slot or the other
// slots (k_spmm's invariance; the lockstep solver relies on it).  No LDS beyond the block sum, no
// scratch (DESIGN.md §3.10 has the register table).
#include "device_common.h"

namespace hgm {

template <int NV>
__device__ __forceinline__ void mv_load(const double* X, int64_t i, double (&x)[NV]) {
    const double* p = X + i * NV;
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

template <int NV>
__device__ __forceinline__ void mv_store(double* X, int64_t i, const double (&x)[NV]) {
    double* p = X + i * NV;
    if constexpr (NV == 1) {
        p[0] = x[0];
    } else {
#pragma unroll
        for (int t = 0; t < NV / 2; ++t) {
            nd2 v;
            v.x = x[2 * t];
            v.y = x[2 * t + 1];
            *reinterpret_cast<nd2*>(p + 2 * t) = v;
        }
    }
}

// the terms of the per-slot sums for one row: o^2, or (o - d)^2 with d from D (interleaved or shared)
template <int NV>
__device__ __forceinline__ void mv_sum_terms(int sum, const double* D, int64_t i, const double (&o)[NV],
                                             double (&acc)[NV]) {
    if (sum == MVS_SQ) {
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const double p = o[r] * o[r];
            acc[r] += p;
        }
    } else if (sum == MVS_DIFF) {
        double d[NV];
        mv_load<NV>(D, i, d);
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const double e = o[r] - d[r];
            const double p = e * e;
            acc[r] += p;
        }
    } else if (sum == MVS_DIFF_SHARED) {
        const double d = D[i];
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            const double e = o[r] - d;
            const double p = e * e;
            acc[r] += p;
        }
    }
}

// parts[r * gridDim.x + blockIdx.x] = the block's sum of slot r (block_sum_all's order per slot)
template <int NV>
__device__ __forceinline__ void mv_sum_tail(double (&acc)[NV], double* parts) {
    __shared__ double sh[NV * 4];
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = wave_sum(acc[r]);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int r = 0; r < NV; ++r) sh[r * 4 + w] = acc[r];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const double* s = sh + threadIdx.x * 4;
        parts[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

struct MvLinArgs {
    const double *X, *Y, *Z, *D;
    double* Out;
    MvCoef a, b, c;
};

template <int NV, int NT>
__global__ __launch_bounds__(BS) void k_mv_lin(int64_t n, MvLinArgs A, int sum, double* parts) {
    double acc[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double x[NV], o[NV];
        mv_load<NV>(A.X, i, x);
#pragma unroll
        for (int r = 0; r < NV; ++r) o[r] = A.a.c[r] * x[r];
        if constexpr (NT >= 2) {
            mv_load<NV>(A.Y, i, x);
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const double p = A.b.c[r] * x[r];
                o[r] = o[r] + p;
            }
        }
        if constexpr (NT >= 3) {
            mv_load<NV>(A.Z, i, x);
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const double p = A.c.c[r] * x[r];
                o[r] = o[r] + p;
            }
        }
        if (A.Out) mv_store<NV>(A.Out, i, o);
        mv_sum_terms<NV>(sum, A.D, i, o, acc);
    }
    if (sum != MVS_NONE) mv_sum_tail<NV>(acc, parts);
}

template <int NV>
__global__ __launch_bounds__(BS) void k_mv_div(int64_t n, const double* In, double* Out, MvCoef s, int guard) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double x[NV];
        mv_load<NV>(In, i, x);
#pragma unroll
        for (int r = 0; r < NV; ++r)
            if (!guard || s.c[r] > 0.0) x[r] = x[r] / s.c[r];
        mv_store<NV>(Out, i, x);
    }
}

template <int NV>
__global__ __launch_bounds__(BS) void k_mv_lsqr_step(int64_t n, double* V, double* X, double* W, MvCoef alpha,
                                                     MvCoef cx, MvCoef cw, int sum, const double* D, double* parts) {
    double acc[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double v[NV], x[NV], w[NV];
        mv_load<NV>(V, i, v);
        mv_load<NV>(X, i, x);
        mv_load<NV>(W, i, w);
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            v[r] = v[r] / alpha.c[r];                       // :28
            const double p = cx.c[r] * w[r];
            x[r] = x[r] + p;                                // :40
            const double q = cw.c[r] * w[r];
            w[r] = v[r] - q;                                // :41
        }
        mv_store<NV>(V, i, v);
        mv_store<NV>(X, i, x);
        mv_store<NV>(W, i, w);
        mv_sum_terms<NV>(sum, D, i, x, acc);                // :43
    }
    if (sum != MVS_NONE) mv_sum_tail<NV>(acc, parts);
}

template <int NV>
__global__ __launch_bounds__(BS) void k_mv_lsmr_step(int64_t n, double* V, double* X, double* H, double* HB,
                                                     MvCoef alpha, MvCoef chb, MvCoef cx, MvCoef ch, int first,
                                                     int sum, const double* D, double* parts) {
    double acc[NV];
#pragma unroll
    for (int r = 0; r < NV; ++r) acc[r] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double v[NV], x[NV], h[NV], hb[NV];
        mv_load<NV>(V, i, v);
        mv_load<NV>(X, i, x);
        mv_load<NV>(H, i, h);
        if (!first) mv_load<NV>(HB, i, hb);
#pragma unroll
        for (int r = 0; r < NV; ++r) {
            if (alpha.c[r] > 0.0) v[r] = v[r] / alpha.c[r];   // :40
            if (first) {
                hb[r] = h[r];                               // :62
            } else {
                const double p = chb.c[r] * hb[r];
                hb[r] = h[r] - p;                           // :64
            }
            const double q = cx.c[r] * hb[r];
            x[r] = x[r] + q;                                // :66
            const double t = ch.c[r] * h[r];
            h[r] = v[r] - t;                                // :67
        }
        mv_store<NV>(V, i, v);
        mv_store<NV>(X, i, x);
        mv_store<NV>(H, i, h);
        mv_store<NV>(HB, i, hb);
        mv_sum_terms<NV>(sum, D, i, x, acc);                // :72
    }
    if (sum != MVS_NONE) mv_sum_tail<NV>(acc, parts);
}

// Out(i, r) = src.p[r][i * src.stride[r]] (slot r of the new group: one slot of an old group of width
// stride[r]); a null source writes zeros.  Out must not overlap a source.
template <int NV>
__global__ __launch_bounds__(BS) void k_mv_regather(int64_t n, MvSlots src, double* __restrict__ Out) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double x[NV];
#pragma unroll
        for (int r = 0; r < NV; ++r) x[r] = src.p[r] ? src.p[r][i * src.stride[r]] : 0.0;
        mv_store<NV>(Out, i, x);
    }
}

// out[slot] = sum of parts[slot][0 .. np) in k_finalize's order; one block per slot
__global__ __launch_bounds__(BS) void k_mv_finalize(const double* __restrict__ parts, int np, double* out) {
    __shared__ double sh[4];
    const double r = reduce_parts<double, false>(parts + (int64_t)blockIdx.x * np, np, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

// Blocks of every kernel here, and the partials per slot: from the length alone.  Past
// MAX_PARTS * BS rows a thread strides over several rows.
int gkmv_grid(int64_t n) {
    int64_t nb = (n + BS - 1) / BS;
    if (nb > MAX_PARTS) nb = MAX_PARTS;
    return (int)(nb < 1 ? 1 : nb);
}

static void check_nvec(int nvec) { HGM_REQUIRE(nvec >= 1 && nvec <= SPMM_MAXV, "gkmv: 1 <= nvec <= 8"); }

// the sums of a launch that left parts[NV][np]; an empty vector sums to zero
static void mv_finish_sums(hgm_ctx* c, int64_t n, int NV, int sum, const double* parts, int np, double* sums) {
    if (sum == MVS_NONE || !sums) return;
    if (n <= 0) {
        HGM_HIP(hipMemsetAsync(sums, 0, sizeof(double) * NV, c->stream));
        return;
    }
    launch(c, false, k_mv_finalize, dim3(NV), dim3(BS), parts, np, sums);
}

static MvWidths width_of(int nvec) { return MvWidths{spmm_width(nvec)}; }
using LinTerms = Ints<1, 2, 3>;   // terms of mv_lin's linear form

void mv_lin(hgm_ctx* c, int64_t n, int nvec, const MvLin& L) {
    check_nvec(nvec);
    HGM_REQUIRE(L.nterms >= 1 && L.nterms <= 3, "mv_lin: 1 to 3 terms");
    HGM_REQUIRE(L.sum == MVS_NONE || L.sums != nullptr, "mv_lin: the sums need a destination");
    HGM_REQUIRE(L.sum == MVS_NONE || L.sum == MVS_SQ || L.D != nullptr, "mv_lin: the difference sums need D");
    const int np = gkmv_grid(n);
    double* parts = L.sum != MVS_NONE ? c->buf<double>("gkmv_parts", (size_t)SPMM_MAXV * MAX_PARTS) : nullptr;
    if (n > 0) {
        MvLinArgs A{L.X, L.Y, L.Z, L.D, L.Out, L.a, L.b, L.c};
        const dim3 g(np), b(BS);
        dispatch([&](auto nv, auto nt) { launch(c, false, k_mv_lin<nv, nt>, g, b, n, A, L.sum, parts); }, width_of(nvec),
                 LinTerms{L.nterms});
    }
    mv_finish_sums(c, n, spmm_width(nvec), L.sum, parts, np, L.sums);
    HGM_HIP(hipGetLastError());
}

void mv_div(hgm_ctx* c, int64_t n, int nvec, const double* In, double* Out, const MvCoef& s, bool guard) {
    check_nvec(nvec);
    if (n <= 0) return;
    const dim3 g(gkmv_grid(n)), b(BS);
    dispatch([&](auto nv) { launch(c, false, k_mv_div<nv>, g, b, n, In, Out, s, guard ? 1 : 0); }, width_of(nvec));
    HGM_HIP(hipGetLastError());
}

void mv_lsqr_step(hgm_ctx* c, int64_t n, int nvec, double* V, double* X, double* W, const MvCoef& alpha,
                  const MvCoef& cx, const MvCoef& cw, int sum, const double* D, double* sums) {
    check_nvec(nvec);
    const int np = gkmv_grid(n);
    double* parts = sum != MVS_NONE ? c->buf<double>("gkmv_parts", (size_t)SPMM_MAXV * MAX_PARTS) : nullptr;
    if (n > 0) {
        const dim3 g(np), b(BS);
        dispatch([&](auto nv) { launch(c, false, k_mv_lsqr_step<nv>, g, b, n, V, X, W, alpha, cx, cw, sum, D, parts); },
                 width_of(nvec));
    }
    mv_finish_sums(c, n, spmm_width(nvec), sum, parts, np, sums);
    HGM_HIP(hipGetLastError());
}

void mv_lsmr_step(hgm_ctx* c, int64_t n, int nvec, double* V, double* X, double* H, double* HB, const MvCoef& alpha,
                  const MvCoef& chb, const MvCoef& cx, const MvCoef& ch, bool first, int sum, const double* D,
                  double* sums) {
    check_nvec(nvec);
    const int np = gkmv_grid(n);
    double* parts = sum != MVS_NONE ? c->buf<double>("gkmv_parts", (size_t)SPMM_MAXV * MAX_PARTS) : nullptr;
    if (n > 0) {
        const dim3 g(np), b(BS);
        dispatch(
            [&](auto nv) {
                launch(c, false, k_mv_lsmr_step<nv>, g, b, n, V, X, H, HB, alpha, chb, cx, ch, first ? 1 : 0, sum, D,
                       parts);
            },
            width_of(nvec));
    }
    mv_finish_sums(c, n, spmm_width(nvec), sum, parts, np, sums);
    HGM_HIP(hipGetLastError());
}

void mv_regather(hgm_ctx* c, int64_t n, int nvec, const MvSlots& src, double* Out) {
    check_nvec(nvec);
    if (n <= 0) return;
    const dim3 g(gkmv_grid(n)), b(BS);
    dispatch([&](auto nv) { launch(c, false, k_mv_regather<nv>, g, b, n, src, Out); }, width_of(nvec));
    HGM_HIP(hipGetLastError());
}

}  // namespace hgm
