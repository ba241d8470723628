// Device code of the Golub-Kahan solvers (lsqr_solver.m, lsmr_solver.m), written for gfx950
// (CDNA4): the elementwise recurrences with their fused partial sums, the one-thread rotation
// kernels (the arithmetic itself is internal.h lsqr_rotate / lsmr_rotate, shared with the host
// loops), the m-space half of the one-pass step and the kept-product monitors.  Each recurrence
// has one element body; the host-scalar, device-scalar and fused kernels all call it, so their
// bits agree by construction.  The library is built with -ffp-contract=off: every temporary below
// that splits a product from a sum is one of MATLAB's two roundings.
#include "device_common.h"

namespace hgm {

// this block's sum of acc into parts[blockIdx.x]
template <typename T>
__device__ __forceinline__ void block_part(T acc, T* sh, T* __restrict__ parts) {
    const T tot = block_sum_all(acc, sh);
    if (threadIdx.x == 0) parts[blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------
// Ridden scalars (internal.h ScalarCopy)
// ------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void scalar_copies(const ScalarCopy<T>& cp) {
    if (cp.dst) *cp.dst = *cp.src;
    if (cp.ddst) *cp.ddst = *cp.dsrc;
}
template <typename T>
__global__ void k_copy_scalars(ScalarCopy<T> cp) {
    if (threadIdx.x == 0 && blockIdx.x == 0) scalar_copies(cp);
}
template <typename T>
void copy_scalars(hgm_ctx* c, const ScalarCopy<T>& cp) {
    k_copy_scalars<T><<<1, 64, 0, c->stream>>>(cp);
    HGM_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------
// out = in / s, s = (T)sqrt((double)sum).  PARTS: the sum is re-formed from np partials by every
// block in k_finalize's order (reduce_parts: the same bits) and block 0 publishes it to ss_out --
// the one-pass m-space step's division, in place of a k_finalize + division launch pair; else the
// sum is *ss.  NZ: a zero s leaves in (lsmr_solver.m:36: if beta > 0, u = u / beta).
// ------------------------------------------------------------------------------
template <typename T, bool PARTS, bool NZ>
__global__ __launch_bounds__(BS) void k_div_sqrt(int64_t n, const T* __restrict__ in, T* __restrict__ out,
                                                 const T* __restrict__ ss, int np, T* ss_out) {
    T ssv;
    if constexpr (PARTS) {
        __shared__ T sh[4];
        ssv = reduce_parts(ss, np, sh);
        if (blockIdx.x == 0 && threadIdx.x == 0) st_sys(ss_out, ssv);
    } else {
        ssv = *ss;
    }
    const T s = (T)sqrt((double)ssv);
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS)
        out[i] = (!NZ || s > T(0)) ? in[i] / s : in[i];
}
template <typename T, bool PARTS>
static void div_sqrt_launch(hgm_ctx* c, int64_t n, const T* in, T* out, const T* ss, int np, T* ss_out, bool nz) {
    if (nz) k_div_sqrt<T, PARTS, true><<<grid_for(n), BS, 0, c->stream>>>(n, in, out, ss, np, ss_out);
    else k_div_sqrt<T, PARTS, false><<<grid_for(n), BS, 0, c->stream>>>(n, in, out, ss, np, ss_out);
    HGM_HIP(hipGetLastError());
}
template <typename T>
void div_sqrt(hgm_ctx* c, int64_t n, const T* in, T* out, const T* ss) {
    div_sqrt_launch<T, false>(c, n, in, out, ss, 0, nullptr, false);
}
template <typename T>
void div_sqrt_nz(hgm_ctx* c, int64_t n, const T* in, T* out, const T* ss) {
    div_sqrt_launch<T, false>(c, n, in, out, ss, 0, nullptr, true);
}

// ------------------------------------------------------------------------------
// LSQR
// ------------------------------------------------------------------------------
// lsqr_solver.m:40-41 for one element:  x = x + (phi/rho) w ;  w = v - (theta/rho) w
template <typename T>
__device__ __forceinline__ void lsqr_upd(T& x, T& w, T v, T a, T b) {
    const T p = a * w;
    x = x + p;
    const T q = b * w;
    w = v - q;
}

// The step on the W elements from i: v = v / alpha (:28), then :40-41 when live, and with err the
// terms of ||x - x_true||^2 (:43) added to acc.
template <typename T, int W>
__device__ __forceinline__ void lsqr_step_elems(int64_t i, T* x, T* w, T* v,
                                                const T* xt, T alpha, T a, T b, bool live, bool err,
                                                T& acc) {
    T vv[W], xx[W], ww[W], tt[W];
    vload<W>(v, i, vv);
    vload<W>(x, i, xx);
    if (live) vload<W>(w, i, ww);
    if (err) vload<W>(xt, i, tt);
#pragma unroll
    for (int e = 0; e < W; ++e) {
        vv[e] = vv[e] / alpha;
        if (live) lsqr_upd(xx[e], ww[e], vv[e], a, b);
        if (err) {
            const T d = xx[e] - tt[e];
            acc += d * d;
        }
    }
    vstore<W>(v, i, vv);
    if (live) {
        vstore<W>(x, i, xx);
        vstore<W>(w, i, ww);
    }
}

// :40-41 with host scalars
template <typename T>
__global__ __launch_bounds__(BS) void k_lsqr_update(int64_t n, T* __restrict__ x, T* __restrict__ w,
                                                    const T* __restrict__ v, T a, T b) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        T wi = w[i], xi = x[i];
        lsqr_upd(xi, wi, v[i], a, b);
        x[i] = xi;
        w[i] = wi;
    }
}
template <typename T> void lsqr_update(hgm_ctx* c, int64_t n, T* x, T* w, const T* v, T a, T b) {
    k_lsqr_update<T><<<grid_for(n), BS, 0, c->stream>>>(n, x, w, v, a, b);
    HGM_HIP(hipGetLastError());
}

// Device-resident LSQR scalars (lsqr_solver.m:22-46 without host round trips): the Givens
// rotation of :31-38 in one thread (lsqr_rotate, the host loop's function), from the sums of
// squares *ssb = beta^2 and *ssa = alpha^2, and the stop test of :44-46 as a flag the step kernel
// honours.  st: [rho_bar, phi_bar, stop] (stop = iteration+1 of the first res <= tol, 0 while
// running).
template <typename T>
__global__ void k_lsqr_rot(const T* ssb, const T* ssa, double* st, T* coef, double* phib_hist, int k, double nb,
                           double tol, ScalarCopy<T> cp) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    scalar_copies(cp);
    const double beta = sqrt((double)*ssb);                  // :23
    const double alpha = sqrt((double)*ssa);                 // :27
    double rho_bar = st[0], phi_bar = st[1], c_x, c_w;
    lsqr_rotate(beta, alpha, rho_bar, phi_bar, c_x, c_w);    // :31-38
    st[0] = rho_bar;
    st[1] = phi_bar;
    coef[0] = (T)c_x;                                        // :40
    coef[1] = (T)c_w;                                        // :41
    phib_hist[k] = phi_bar;
    if (st[2] == 0.0 && fabs(phi_bar) / nb <= tol) st[2] = (double)(k + 1);   // :44-46
}
template <typename T>
void lsqr_rot(hgm_ctx* c, const T* ssb, const T* ssa, double* st, T* coef, double* phib_hist, int k, double nb,
              double tol, const ScalarCopy<T>& cp) {
    k_lsqr_rot<T><<<1, 64, 0, c->stream>>>(ssb, ssa, st, coef, phib_hist, k, nb, tol, cp);
    HGM_HIP(hipGetLastError());
}

// v = v_hat / alpha (alpha = sqrt(*ssa)), then x += (phi/rho) w ; w = v - (theta/rho) w
// (lsqr_solver.m:28,40-41), skipped once an earlier iteration met the stop test; with parts,
// also the partials of ||x - x_true||^2 (:43) in k_reduce_partial<T, 2>'s order (same bits).
template <typename T, bool VEC>
__global__ __launch_bounds__(BS) void k_lsqr_step(int64_t n, T* __restrict__ x, T* __restrict__ w, T* __restrict__ v,
                                                  const T* ssa, const T* coef, const double* st, int k,
                                                  const T* __restrict__ xt, T* __restrict__ parts) {
    __shared__ T sh[4];
    const T alpha = (T)sqrt((double)*ssa);
    const bool live = !(st[2] != 0.0 && st[2] < (double)(k + 1));
    const T a = coef[0], b = coef[1];
    T acc = 0;
    grid_elems<T, VEC>(n, [&](int64_t i, auto wc) {
        lsqr_step_elems<T, decltype(wc)::value>(i, x, w, v, xt, alpha, a, b, live, parts != nullptr, acc);
    });
    if (parts) block_part(acc, sh, parts);
}
template <typename T>
void lsqr_step(hgm_ctx* c, int64_t n, T* x, T* w, T* v, const T* ssa, const T* coef, const double* st, int k,
               const T* xt, T* err_out) {
    // (vectors as k_reduce_partial takes them for the same x and x_true: the same error bits)
    const SumParts<T> s = launch_sum<T>(c, n, xt ? SUM_LONG : SUM_NONE, "red_parts", err_out,
                                        [&](auto vec, int np, T* parts) {
        k_lsqr_step<T, decltype(vec)::value><<<np, BS, 0, c->stream>>>(n, x, w, v, ssa, coef, st, k, xt, parts);
    }, x, w, v, xt);
    if (xt && !s.fuse) sumsq_diff<T>(c, n, x, xt, err_out);
}

// (one-pass LSQR) the images of x and w under A, in double, so the exact final residual of
// lsqr_solver.m:52 needs no SpMV: with A*v_{k+1} = w_m / alpha_{k+1} (the pass's A*v_hat),
// A*x += (phi/rho) A*w ; A*w = A*v_{k+1} - (theta/rho) A*w (:40-41 under A).  init: A*w = A*v_0,
// A*x = 0.  Iterations enqueued past a device stop (st[2], as k_lsqr_step) change nothing.
template <typename T>
__global__ __launch_bounds__(BS) void k_lsqr_img(int64_t m, const T* __restrict__ wm, const T* ssa, const T* coef,
                                                 const double* st, int k, double* __restrict__ ax,
                                                 double* __restrict__ aw, int init) {
    const double a = (double)(T)sqrt((double)*ssa);
    const bool live = init || !(st[2] != 0.0 && st[2] < (double)(k + 1));
    if (!live) return;
    const double c0 = init ? 0.0 : (double)coef[0], c1 = init ? 0.0 : (double)coef[1];
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < m; i += (int64_t)gridDim.x * BS) {
        const double av = a != 0.0 ? (double)wm[i] / a : (double)wm[i];
        if (init) {
            ax[i] = 0.0;
            aw[i] = av;
        } else {
            ax[i] = ax[i] + c0 * aw[i];
            aw[i] = av - c1 * aw[i];
        }
    }
}
template <typename T>
void lsqr_img(hgm_ctx* c, int64_t m, const T* wm, const T* ssa, const T* coef, const double* st, int k, double* ax,
              double* aw, bool init) {
    k_lsqr_img<T><<<grid_for(m), BS, 0, c->stream>>>(m, wm, ssa, coef, st, k, ax, aw, init ? 1 : 0);
    HGM_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------
// The m-space half of a Golub-Kahan step after the one-pass w = A*(A'*u - beta*v) (fused.hip):
// A*v_k = w / alpha_k (alpha = (T)sqrt((double)*ssa); a zero alpha leaves w, as lsmr_solver.m:16/40
// leave v undivided), kept in av when given, then t = A*v_k - alpha*u (lsqr_solver.m:22,
// lsmr_solver.m:34; two roundings, as the two-pass EPI_SUB epilogue), with the partials of ||t||^2
// in k_reduce_partial<T, 1>'s layout (parts == nullptr: none).
// ------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(BS) void k_gkb_mstep(int64_t n, const T* __restrict__ w, const T* ssa,
                                                  const T* __restrict__ u, T* __restrict__ t, T* __restrict__ av,
                                                  T* __restrict__ parts) {
    __shared__ T sh[4];
    const T a = (T)sqrt((double)*ssa);
    T acc = 0;
    grid_elems<T, VEC>(n, [&](int64_t i, auto wc) {
        constexpr int W = decltype(wc)::value;
        T ww[W], uu[W], tt[W];
        vload<W>(w, i, ww);
        vload<W>(u, i, uu);
#pragma unroll
        for (int e = 0; e < W; ++e) {
            ww[e] = a != T(0) ? ww[e] / a : ww[e];
            const T s = a * uu[e];
            tt[e] = ww[e] - s;
            acc += tt[e] * tt[e];
        }
        if (av) vstore<W>(av, i, ww);
        vstore<W>(t, i, tt);
    });
    if (parts) block_part(acc, sh, parts);
}
// the step with its partials; fin_out: the finalised ||t||^2 (nullptr: left to the caller)
template <typename T>
static SumParts<T> mstep_launch(hgm_ctx* c, int64_t n, const T* w, const T* ssa, const T* u, T* t, T* av,
                                T* fin_out) {
    return launch_sum<T>(c, n, SUM_LONG, "red_parts", fin_out, [&](auto vec, int np, T* parts) {
        k_gkb_mstep<T, decltype(vec)::value><<<np, BS, 0, c->stream>>>(n, w, ssa, u, t, av, parts);
    }, w, u, t, av);
}
template <typename T>
void gkb_mstep(hgm_ctx* c, int64_t n, const T* w, const T* ssa, const T* u, T* t, T* av, T* ss_out) {
    if (!mstep_launch<T>(c, n, w, ssa, u, t, av, ss_out).fuse) sumsq<T>(c, n, t, ss_out);
}
// gkb_mstep (t = A*v_k - alpha*u, ||t||^2 -> ss_out) followed by u = t / sqrt(||t||^2) (nz: as
// div_sqrt_nz): two launches where the separate calls take three (the same bits).
template <typename T>
void gkb_mstep_div(hgm_ctx* c, int64_t n, const T* w, const T* ssa, T* u, T* t, T* av, T* ss_out, bool nz) {
    const SumParts<T> s = mstep_launch<T>(c, n, w, ssa, u, t, av, nullptr);
    if (s.fuse) {
        div_sqrt_launch<T, true>(c, n, t, u, s.parts, s.np, ss_out, nz);
    } else {
        sumsq<T>(c, n, t, ss_out);
        div_sqrt_launch<T, false>(c, n, t, u, ss_out, 0, nullptr, nz);
    }
}

// ------------------------------------------------------------------------------
// LSMR
// ------------------------------------------------------------------------------
// lsmr_solver.m:61-67 for one element: hbar = h - c_hbar hbar (FIRST: hbar = h, :62), x += c_x hbar,
// h = v - c_h h
template <typename T, bool FIRST>
__device__ __forceinline__ void lsmr_upd(T& x, T& h, T& hb, T v, T c_hbar, T c_x, T c_h) {
    if (FIRST) hb = h;                                   // :62
    else { const T p = c_hbar * hb; hb = h - p; }        // :64
    const T q = c_x * hb;
    x = x + q;                                           // :66
    const T r = c_h * h;
    h = v - r;                                           // :67
}

// The n-space step on the W elements from i: v = v / alpha unless alpha is zero (:40), then :61-67
// when live, and with err the terms of ||x - x_true||^2 (:72) added to acc.
template <typename T, bool FIRST, int W>
__device__ __forceinline__ void lsmr_step_elems(int64_t i, T* x, T* h, T* hbar,
                                                T* v, const T* xt, T alpha, T c_hbar,
                                                T c_x, T c_h, bool live, bool err, T& acc) {
    T vv[W], xx[W], hh[W], hb[W], tt[W];
    vload<W>(v, i, vv);
    vload<W>(x, i, xx);
    if (live) {
        vload<W>(h, i, hh);
        if (!FIRST) vload<W>(hbar, i, hb);
    }
    if (err) vload<W>(xt, i, tt);
#pragma unroll
    for (int e = 0; e < W; ++e) {
        if (alpha > T(0)) vv[e] = vv[e] / alpha;         // :40
        if (live) lsmr_upd<T, FIRST>(xx[e], hh[e], hb[e], vv[e], c_hbar, c_x, c_h);
        if (err) {
            const T d = xx[e] - tt[e];
            acc += d * d;
        }
    }
    if (alpha > T(0)) vstore<W>(v, i, vv);
    if (live) {
        vstore<W>(hbar, i, hb);
        vstore<W>(x, i, xx);
        vstore<W>(h, i, hh);
    }
}

// The image recurrences of the kept-product monitors for one element, in double:
// image(h_k) = iv - f image(h_{k-1}), image(hbar_k) = image(h_k) - e image(hbar_{k-1}); FIRST:
// h_0 = v_0 (:25), hbar_0 = h_0 (:62).
template <bool FIRST>
__device__ __forceinline__ void lsmr_img_rec(double iv, double h_prev, double hb_prev, double f, double e,
                                             double& ih, double& ihb) {
    if (FIRST) {
        ih = iv;
        ihb = ih;
    } else {
        const double q = f * h_prev;
        ih = iv - q;
        const double w = e * hb_prev;
        ihb = ih - w;
    }
}

// The carried-residual n-space monitor on the W elements from i (k_lsmr_mon_r): image of
// v_k = c1 p1 + c0 p0, the recurrences above, Ir = Ir - cx image(hbar_k), all updated in double and
// stored in T; the squares of the stored Ir added to acc.
template <typename T, bool FIRST, int W>
__device__ __forceinline__ void lsmr_monr_elems(int64_t i, const T* p1, const T* p0,
                                                T* Ih, T* Ihb, T* Ir,
                                                double c1, double c0, double f, double e, double cx, double& acc) {
    T a[W], b[W], h[W], hb[W], r[W];
    vload<W>(p1, i, a);
    vload<W>(p0, i, b);
    if (!FIRST) {
        vload<W>(Ih, i, h);
        vload<W>(Ihb, i, hb);
    }
    vload<W>(Ir, i, r);
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const double x1 = c1 * (double)a[u], x0 = c0 * (double)b[u];
        const double iv = x1 + x0;
        double ih, ihb;
        lsmr_img_rec<FIRST>(iv, FIRST ? 0.0 : (double)h[u], FIRST ? 0.0 : (double)hb[u], f, e, ih, ihb);
        const double s = cx * ihb;
        const double ir = (double)r[u] - s;
        h[u] = (T)ih;
        hb[u] = (T)ihb;
        r[u] = (T)ir;
        const double rr = (double)r[u];
        acc += rr * rr;
    }
    vstore<W>(Ih, i, h);
    vstore<W>(Ihb, i, hb);
    vstore<W>(Ir, i, r);
}

// :61-67 with host scalars
template <typename T, bool FIRST>
__global__ __launch_bounds__(BS) void k_lsmr_update(int64_t n, T* __restrict__ x, T* __restrict__ h,
                                                    T* __restrict__ hbar, const T* __restrict__ v,
                                                    T c_hbar, T c_x, T c_h) {
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        T hi = h[i], hb = FIRST ? T(0) : hbar[i], xi = x[i];
        lsmr_upd<T, FIRST>(xi, hi, hb, v[i], c_hbar, c_x, c_h);
        hbar[i] = hb;
        x[i] = xi;
        h[i] = hi;
    }
}
template <typename T>
void lsmr_update(hgm_ctx* c, int64_t n, T* x, T* h, T* hbar, const T* v, T c_hbar, T c_x, T c_h, bool first) {
    if (first) k_lsmr_update<T, true><<<grid_for(n), BS, 0, c->stream>>>(n, x, h, hbar, v, c_hbar, c_x, c_h);
    else k_lsmr_update<T, false><<<grid_for(n), BS, 0, c->stream>>>(n, x, h, hbar, v, c_hbar, c_x, c_h);
    HGM_HIP(hipGetLastError());
}

// Device-resident LSMR scalars (lsmr_solver.m:42-67): lsmr_rotate, the host loop's function, in one
// thread.  st = [alpha, alphabar, rho, rhobar, cbar, sbar, zetabar, prev (theta/rho), stop];
// *ssb = beta^2, *ssa = alpha^2 of this step.  coef = (T)[c_hbar, c_x, c_h] of :64/:66/:67 for the
// n-space update; cfm / cfn = the monitors' coefficients [c1, c0, f, e, cx] (m-space: image of
// v = A*v_k; n-space: beta A'u_{k+1} + alpha_k A'u_k).
template <typename T>
__global__ void k_lsmr_rot(const T* ssb, const T* ssa, double* st, T* coef, double* cfm, double* cfn,
                           ScalarCopy<T> cp) {
    if (threadIdx.x != 0) return;
    scalar_copies(cp);
    const double beta = sqrt((double)*ssb), alpha = sqrt((double)*ssa);   // :35, :39
    double c3[3];
    lsmr_rotate(beta, alpha, st, c3, cfm, cfn);
    coef[0] = (T)c3[0];
    coef[1] = (T)c3[1];
    coef[2] = (T)c3[2];
}
template <typename T>
void lsmr_rot(hgm_ctx* c, const T* ssb, const T* ssa, double* st, T* coef, double* cfm, double* cfn,
              const ScalarCopy<T>& cp) {
    k_lsmr_rot<T><<<1, 64, 0, c->stream>>>(ssb, ssa, st, coef, cfm, cfn, cp);
    HGM_HIP(hipGetLastError());
}

// The n-space LSMR step (lsmr_solver.m:40, :61-67) with device coefficients: v = v / alpha
// (alpha = (T)sqrt(*ssa); a zero alpha leaves v, :40), hbar = h - c_hbar hbar (k = 0: h), x += c_x hbar,
// h = v - c_h h -- x, h, hbar untouched once an earlier iteration met the stop test -- and, with
// parts, the partials of ||x - x_true||^2 (:72) in k_lsqr_step's layout.
template <typename T, bool FIRST, bool VEC>
__global__ __launch_bounds__(BS) void k_lsmr_step(int64_t n, T* __restrict__ x, T* __restrict__ h,
                                                  T* __restrict__ hbar, T* __restrict__ v, const T* ssa,
                                                  const T* coef, const double* st, int k, const T* __restrict__ xt,
                                                  T* __restrict__ parts) {
    __shared__ T sh[4];
    const T alpha = (T)sqrt((double)*ssa);
    const bool live = !(st[8] != 0.0 && st[8] < (double)(k + 1));
    const T c_hbar = coef[0], c_x = coef[1], c_h = coef[2];
    T acc = 0;
    grid_elems<T, VEC>(n, [&](int64_t i, auto wc) {
        lsmr_step_elems<T, FIRST, decltype(wc)::value>(i, x, h, hbar, v, xt, alpha, c_hbar, c_x, c_h, live,
                                                       parts != nullptr, acc);
    });
    if (parts) block_part(acc, sh, parts);
}
template <typename T>
void lsmr_step(hgm_ctx* c, int64_t n, T* x, T* h, T* hbar, T* v, const T* ssa, const T* coef, const double* st,
               int k, const T* xt, T* err_out) {
    const SumParts<T> s = launch_sum<T>(c, n, xt ? SUM_LONG : SUM_NONE, "red_parts", err_out,
                                        [&](auto vec, int np, T* parts) {
        constexpr bool V = decltype(vec)::value;
        if (k == 0) k_lsmr_step<T, true, V><<<np, BS, 0, c->stream>>>(n, x, h, hbar, v, ssa, coef, st, k, xt, parts);
        else k_lsmr_step<T, false, V><<<np, BS, 0, c->stream>>>(n, x, h, hbar, v, ssa, coef, st, k, xt, parts);
    }, x, h, hbar, v, xt);
    if (xt && !s.fuse) sumsq_diff<T>(c, n, x, xt, err_out);
}

// :76 on the device: st[8] = k + 1 at the first iteration with sqrt(||r||^2) / (||b|| + eps) < tol
__global__ void k_lsmr_stop(const double* rr, double nb, double tol, double* st, int k) {
    if (threadIdx.x != 0) return;
    const double res = sqrt(rr[0]) / (nb + 0x1p-52);   // eps
    if (st[8] == 0.0 && res < tol) st[8] = (double)(k + 1);
}
void lsmr_stop(hgm_ctx* c, const double* rr, double nb, double tol, double* st, int k) {
    k_lsmr_stop<<<1, 64, 0, c->stream>>>(rr, nb, tol, st, k);
    HGM_HIP(hipGetLastError());
}

// LSMR monitors from kept products.  The images of the LSMR vectors under A
// and A'A follow the same recurrences as the vectors (lsmr_solver.m:61-67), fed by the raw
// products the bidiagonalisation already forms:
//   m-space: A*h_k = A*v_k - f*A*h_{k-1};  A*hbar_k = A*h_k - e*A*hbar_{k-1};  A*x_k = A*x_{k-1} + cx*A*hbar_k
//   n-space: A'A*v_k = beta_{k+1} A'u_{k+1} + alpha_k A'u_k  (A*v_k = beta_{k+1} u_{k+1} + alpha_k u_k,
//            lsmr_solver.m:34-36), then the same three updates for A'A*h, A'A*hbar, A'A*x.
// r = b - A*x (:69) and A'r = A'b - A'A*x (:71) are then norms of kept vectors.  The images are
// accumulated in fp64 for both value types.  parts[blk] = this block's sum of the squared
// monitor vector.
// cf != NULL: the coefficients [c1, c0, f, e, cx] from the device (k_lsmr_rot) instead of the arguments.
template <typename T, bool FIRST>
__global__ __launch_bounds__(BS) void k_lsmr_mon(int64_t n, const T* __restrict__ p1, const T* __restrict__ p0,
                                                 double c1, double c0, double* __restrict__ Ih,
                                                 double* __restrict__ Ihb, double* __restrict__ Ix,
                                                 const T* __restrict__ rhs, double f, double e, double cx,
                                                 double* __restrict__ parts, const double* __restrict__ cf) {
    __shared__ double sh[4];
    if (cf) {
        c1 = cf[0];
        c0 = cf[1];
        f = cf[2];
        e = cf[3];
        cx = cf[4];
    }
    double acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < n; i += (int64_t)gridDim.x * BS) {
        double iv;                                          // image of v_k
        if (p0) { const double a = c1 * (double)p1[i], b = c0 * (double)p0[i]; iv = a + b; }
        else iv = (double)p1[i];
        double ih, ihb;
        lsmr_img_rec<FIRST>(iv, FIRST ? 0.0 : Ih[i], FIRST ? 0.0 : Ihb[i], f, e, ih, ihb);
        const double s = cx * ihb;
        const double ix = Ix[i] + s;
        Ih[i] = ih;
        Ihb[i] = ihb;
        Ix[i] = ix;
        const double d = (double)rhs[i] - ix;
        acc += d * d;
    }
    block_part(acc, sh, parts);
}
template <typename T>
void lsmr_monitor(hgm_ctx* c, int64_t n, const T* p1, const T* p0, double c1, double c0, double* Ih, double* Ihb,
                  double* Ix, const T* rhs, double f, double e, double cx, bool first, double* out, const double* cf) {
    // (scalar elements: no alignment to test)
    launch_sum<double>(c, n, SUM_ANY, "lsmr_mon_parts", out, [&](auto, int np, double* parts) {
        if (first)
            k_lsmr_mon<T, true><<<np, BS, 0, c->stream>>>(n, p1, p0, c1, c0, Ih, Ihb, Ix, rhs, f, e, cx, parts, cf);
        else
            k_lsmr_mon<T, false><<<np, BS, 0, c->stream>>>(n, p1, p0, c1, c0, Ih, Ihb, Ix, rhs, f, e, cx, parts, cf);
    });
}

// The n-space monitor of the fp32 solves in carried-residual form: the images of h and hbar and
// the normal-equations residual Ir = A'b - A'A*x itself (Ir_0 = A'b) are stored in T and updated in
// double, Ir_k = Ir_{k-1} - cx * image(hbar_k); parts = sum Ir_k^2 (the rounded values carried on).
// Carrying Ir instead of image(x) keeps the small residual from a cancellation against A'b, so T
// storage holds its relative accuracy; it moves 3 T arrays twice plus p1, p0 per iteration instead
// of 3 double arrays twice plus p1, p0 and A'b (C5: 0.54 against 1.0 GB).
template <typename T, bool FIRST, bool VEC>
__global__ __launch_bounds__(BS) void k_lsmr_mon_r(int64_t n, const T* __restrict__ p1, const T* __restrict__ p0,
                                                   T* __restrict__ Ih, T* __restrict__ Ihb, T* __restrict__ Ir,
                                                   double* __restrict__ parts, const double* __restrict__ cf) {
    __shared__ double sh[4];
    const double c1 = cf[0], c0 = cf[1], f = cf[2], e = cf[3], cx = cf[4];
    double acc = 0;
    grid_elems<T, VEC>(n, [&](int64_t i, auto wc) {
        lsmr_monr_elems<T, FIRST, decltype(wc)::value>(i, p1, p0, Ih, Ihb, Ir, c1, c0, f, e, cx, acc);
    });
    block_part(acc, sh, parts);
}
template <typename T>
void lsmr_monitor_r(hgm_ctx* c, int64_t n, const T* p1, const T* p0, T* Ih, T* Ihb, T* Ir, bool first, double* out,
                    const double* cf) {
    launch_sum<double>(c, n, SUM_ANY, "lsmr_mon_parts", out, [&](auto vec, int np, double* parts) {
        constexpr bool V = decltype(vec)::value;
        if (first) k_lsmr_mon_r<T, true, V><<<np, BS, 0, c->stream>>>(n, p1, p0, Ih, Ihb, Ir, parts, cf);
        else k_lsmr_mon_r<T, false, V><<<np, BS, 0, c->stream>>>(n, p1, p0, Ih, Ihb, Ir, parts, cf);
    }, p1, p0, Ih, Ihb, Ir);
}

// k_lsmr_step and k_lsmr_mon_r in one pass over the n-space (the fp32 one-pass LSMR with x_true):
// the two kernels walk the same elements in the same grid (parts_for(n) blocks, grid_elems) and
// touch disjoint vectors, so each of the two block sums -- and every element -- has the bits of
// the two separate launches; one launch boundary and one sweep of the grid instead of two.
template <typename T, bool FIRST>
__global__ __launch_bounds__(BS) void k_lsmr_step_mon(int64_t n, T* __restrict__ x, T* __restrict__ h,
                                                      T* __restrict__ hbar, T* __restrict__ v, const T* ssa,
                                                      const T* coef, const double* st, int k, const T* __restrict__ xt,
                                                      T* __restrict__ parts_e, const T* __restrict__ p1,
                                                      const T* __restrict__ p0, T* __restrict__ Ih, T* __restrict__ Ihb,
                                                      T* __restrict__ Ir, double* __restrict__ parts_m,
                                                      const double* __restrict__ cf) {
    __shared__ T sh[4];
    __shared__ double shm[4];
    const T alpha = (T)sqrt((double)*ssa);
    const bool live = !(st[8] != 0.0 && st[8] < (double)(k + 1));
    const T c_hbar = coef[0], c_x = coef[1], c_h = coef[2];
    const double c1 = cf[0], c0 = cf[1], f = cf[2], e = cf[3], cx = cf[4];
    T acc = 0;
    double accm = 0;
    grid_elems<T, true>(n, [&](int64_t i, auto wc) {
        constexpr int W = decltype(wc)::value;
        lsmr_step_elems<T, FIRST, W>(i, x, h, hbar, v, xt, alpha, c_hbar, c_x, c_h, live, true, acc);
        lsmr_monr_elems<T, FIRST, W>(i, p1, p0, Ih, Ihb, Ir, c1, c0, f, e, cx, accm);
    });
    const T tot = block_sum_all(acc, sh);
    const double totm = block_sum_all(accm, shm);
    if (threadIdx.x == 0) {
        parts_e[blockIdx.x] = tot;
        parts_m[blockIdx.x] = totm;
    }
}

// The fused pair when it gives the separate launches' bits (x_true given, the partial-sum grid,
// 16-byte aligned vectors); false: the caller runs lsmr_step and lsmr_monitor_r.  Two sums from one
// launch, so the plan is launch_sum's and the launch is written out.
template <typename T>
bool lsmr_step_mon(hgm_ctx* c, int64_t n, T* x, T* h, T* hbar, T* v, const T* ssa, const T* coef, const double* st,
                   int k, const T* xt, T* err_out, const T* p1, const T* p0, T* Ih, T* Ihb, T* Ir, bool first,
                   double* mon_out, const double* cf) {
    if (!c->num.lsmr_fuse_nmon) return false;
    const SumPlan s = sum_plan(c, n, xt ? SUM_LONG : SUM_NONE, x, h, hbar, v, xt, p1, p0, Ih, Ihb, Ir);
    if (!s.fuse || !s.vec) return false;
    T* parts_e = c->buf<T>("red_parts", MAX_PARTS);
    double* parts_m = c->buf<double>("lsmr_mon_parts", MAX_PARTS);
    if (first)
        k_lsmr_step_mon<T, true><<<s.np, BS, 0, c->stream>>>(n, x, h, hbar, v, ssa, coef, st, k, xt, parts_e, p1, p0,
                                                             Ih, Ihb, Ir, parts_m, cf);
    else
        k_lsmr_step_mon<T, false><<<s.np, BS, 0, c->stream>>>(n, x, h, hbar, v, ssa, coef, st, k, xt, parts_e, p1, p0,
                                                              Ih, Ihb, Ir, parts_m, cf);
    finalize_parts<T>(c, parts_e, s.np, err_out);
    finalize_parts<double>(c, parts_m, s.np, mon_out);
    HGM_HIP(hipGetLastError());
    return true;
}

// ------------------------------------------------------------------------------
// explicit instantiations
// ------------------------------------------------------------------------------
#define HGM_INST(T)                                                                            \
    template void copy_scalars<T>(hgm_ctx*, const ScalarCopy<T>&);                             \
    template void div_sqrt<T>(hgm_ctx*, int64_t, const T*, T*, const T*);                      \
    template void div_sqrt_nz<T>(hgm_ctx*, int64_t, const T*, T*, const T*);                   \
    template void lsqr_update<T>(hgm_ctx*, int64_t, T*, T*, const T*, T, T);                   \
    template void lsqr_rot<T>(hgm_ctx*, const T*, const T*, double*, T*, double*, int, double, double,   \
                              const ScalarCopy<T>&);                                           \
    template void lsqr_step<T>(hgm_ctx*, int64_t, T*, T*, T*, const T*, const T*, const double*, int, const T*, T*); \
    template void lsqr_img<T>(hgm_ctx*, int64_t, const T*, const T*, const T*, const double*, int, double*, double*, \
                              bool);                                                           \
    template void gkb_mstep<T>(hgm_ctx*, int64_t, const T*, const T*, const T*, T*, T*, T*);   \
    template void gkb_mstep_div<T>(hgm_ctx*, int64_t, const T*, const T*, T*, T*, T*, T*, bool); \
    template void lsmr_update<T>(hgm_ctx*, int64_t, T*, T*, T*, const T*, T, T, T, bool);      \
    template void lsmr_rot<T>(hgm_ctx*, const T*, const T*, double*, T*, double*, double*,     \
                              const ScalarCopy<T>&);                                           \
    template void lsmr_step<T>(hgm_ctx*, int64_t, T*, T*, T*, T*, const T*, const T*, const double*, int, \
                               const T*, T*);                                                  \
    template void lsmr_monitor<T>(hgm_ctx*, int64_t, const T*, const T*, double, double, double*, double*, \
                                  double*, const T*, double, double, double, bool, double*, const double*); \
    template void lsmr_monitor_r<T>(hgm_ctx*, int64_t, const T*, const T*, T*, T*, T*, bool, double*, \
                                    const double*);                                            \
    template bool lsmr_step_mon<T>(hgm_ctx*, int64_t, T*, T*, T*, T*, const T*, const T*, const double*, int, \
                                   const T*, T*, const T*, const T*, T*, T*, T*, bool, double*, const double*);

HGM_INST(double)
HGM_INST(float)

}  // namespace hgm
