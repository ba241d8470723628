// Leading singular triplets of A by Golub-Kahan-Lanczos bidiagonalisation started at b, with full
// reorthogonalisation of both bases (hgm_svds).  It stands where plot_filter_factors.m:30 calls
// [U,S,V] = svd(A,'econ') for the empirical filter factors Phi_emp = sigma .* (V'*x) ./ (U'*b) (:31-40):
// a dense SVD is out of reach at tomography scale, and the modes the figure plots are the leading
// ones that b excites -- the ones a Lanczos run started at b converges to first.
//
//   beta_1 u_1 = b;  for j = 1..k:   v^ = A'u_j - beta_j v_{j-1},      CGS2 against V(:,1:j-1), alpha_j = ||v^||
//                                    u^ = A v_j - alpha_j u_j,         CGS2 against U(:,1:j),   beta_{j+1} = ||u^||
//   one more half step gives alpha_{k+1};  A V_k = U_{k+1} B_k,  B_k = P S Q' (host, dense::bidiag_svd):
//   sigma_i = S_ii,  u~_i = U_{k+1} P(:,i),  v~_i = V_k Q(:,i),  A v~_i = sigma_i u~_i and
//   A'u~_i - sigma_i v~_i = alpha_{k+1} P(k+1,i) v_{k+1}, so resid_i = alpha_{k+1} |P(k+1,i)|;
//   u~_i'b = beta_1 P(1,i) costs nothing because the run starts at b.
//
// The start vector selects the modes: a mode with u_i'b = 0 is never found (the reference would have
// divided by its guard value there), and an exactly repeated singular value comes back once, with the
// projection of b on its singular subspace as the left vector.
//
// The operator passes (classes 0/1), CGS2 (class 2) and the norms are the solvers' kernels; alpha and
// beta stay on the device as sums of squares for the SpMV epilogues (PendNorm::asq), and the host
// reads the step's two scalars once per step for the breakdown test.  The block work on the bases
// afterwards (V_k'X, U_{k+1} P, V_k Q) is basis.hip, one pass each (class 7).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "internal.h"

namespace hgm {

int svds(hgm_ctx* c, const hgm_mat* A, const hgm_mat* At, const double* b_in, int steps, int nsv, double btol,
         const double* X, int64_t ldx, int nx, double* sigma, double* resid, double* utb, double* VtX, double* U_out,
         int64_t ldu_out, double* V_out, int64_t ldv_out, int* steps_done) {
    HGM_REQUIRE(A != nullptr && At != nullptr, "svds: A and At are required");
    HGM_REQUIRE(A->dtype == HGM_F64 && At->dtype == HGM_F64, "svds: fp64 operators only");
    HGM_REQUIRE(!c->num.parity, "svds: not in parity mode");
    HGM_REQUIRE(At->rows == A->cols && At->cols == A->rows, "svds: At must be size(A') (n x m)");
    HGM_REQUIRE(steps >= 1, "svds: steps must be >= 1");
    HGM_REQUIRE(nsv >= 1 && nsv <= steps, "svds: nsv must be in 1..steps");
    HGM_REQUIRE(nx >= 0 && nx <= 64, "svds: nx must be in 0..64");
    HGM_REQUIRE(X == nullptr || VtX != nullptr, "svds: X needs VtX");
    HGM_REQUIRE(nx == 0 || X != nullptr, "svds: nx > 0 needs X");
    HGM_REQUIRE(sigma != nullptr && resid != nullptr && utb != nullptr, "svds: sigma, resid and utb are required");
    const int64_t m = A->rows, n = A->cols;
    HGM_REQUIRE(m >= 1 && n >= 1, "svds: empty operator");
    HGM_REQUIRE(X == nullptr || ldx >= n, "svds: ldx shorter than a column");
    HGM_REQUIRE(U_out == nullptr || ldu_out >= m, "svds: ldu shorter than a column");
    HGM_REQUIRE(V_out == nullptr || ldv_out >= n, "svds: ldv shorter than a column");
    if (dist_n(c) || c->host_ar != nullptr)
        throw Error{HGM_E_UNSUPPORTED, "svds: single rank only (no communicator / all-reduce hook)"};
    HGM_REQUIRE(A->row_order.trivial() && At->col_order.trivial(),
                "the ray (m) space must be stored in the reference order");
    HGM_REQUIRE(At->row_order == A->col_order, "A's columns and At's rows must share one pixel order");
    const PixOrder po = A->col_order;
    const int kmax = (int)std::min<int64_t>(steps, std::min(m, n));
    HGM_REQUIRE(kmax <= 255, "svds: at most 255 steps (the block kernels take bases of up to 256 vectors)");
    if (btol <= 0) btol = 1e-12;
    if (X == nullptr) nx = 0;

    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(sigma, sigma + nsv, nan);
    std::fill(resid, resid + nsv, nan);
    std::fill(utb, utb + nsv, nan);
    if (VtX) std::fill(VtX, VtX + (size_t)nsv * nx, nan);
    if (U_out)
        for (int i = 0; i < nsv; ++i) std::fill(U_out + (size_t)i * ldu_out, U_out + (size_t)i * ldu_out + m, nan);
    if (V_out)
        for (int i = 0; i < nsv; ++i) std::fill(V_out + (size_t)i * ldv_out, V_out + (size_t)i * ldv_out + n, nan);
    if (steps_done) *steps_done = 0;

    // ---- the two bases: (m + n)(steps + 1) doubles ----
    {
        size_t fr = 0, tot = 0;
        HGM_HIP(hipMemGetInfo(&fr, &tot));
        const double need = 8.0 * ((double)krylov_ld(c, m, false) + (double)krylov_ld(c, n, false)) * (kmax + 1);
        if (need > (double)tot)
            throw Error{HGM_E_NOMEM, "svds: the two bases ((m + n)(steps + 1) doubles) do not fit the device"};
    }
    const KrylovBasis kU = krylov_basis(c, "sv_U", m, kmax + 1, false);
    const KrylovBasis kV = krylov_basis(c, "sv_V", n, kmax + 1, false);
    double* Ub = kU.Q;
    double* Vb = kV.Q;
    const int64_t ldu = kU.ld, ldv = kV.ld;
    double* ss = c->buf<double>("sv_ss", (size_t)2 * kmax + 4);     // [beta_1^2 | alpha_j^2, beta_{j+1}^2 ... | alpha_{k+1}^2]
    double* hsink = c->buf<double>("sv_h", (size_t)kmax + 8);       // the CGS2 coefficients (not needed)
    const double* cgs_ss = cgs2_sumsq<double>(c);
    auto keep_ss = [&](double* dst) {
        HGM_HIP(hipMemcpyAsync(dst, cgs_ss, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    };
    auto read2 = [&](const double* dev, int cnt, double* host) {
        Reader rd(c);
        rd.add(host, dev, sizeof(double) * cnt);
        rd.go();
    };

    // ---- beta_1 u_1 = b ----
    double* tv = c->buf<double>("sv_t", (size_t)std::max(m, n) + 1);   // an unnormalised start vector
    if (b_in) h2d(c, tv, b_in, sizeof(double) * m);
    else fill_hash<double>(c, m, tv, 0x5EEDB0A4D5ull);
    sumsq<double>(c, m, tv, ss);
    div_sqrt_nz<double>(c, m, tv, Ub, ss);
    double h2[2] = {0, 0};
    read2(ss, 1, h2);
    const double beta1 = std::sqrt(h2[0]);
    if (!(beta1 > 0)) return HGM_OK;   // b == 0 excites no mode: every output stays NaN

    std::vector<double> alpha(kmax + 1, 0.0), beta(kmax + 1, 0.0);   // alpha[j] = alpha_{j+1}, beta[j] = beta_{j+2}
    double big = 0.0, alpha_next = 0.0;
    bool broke = false;
    int k = 0;
    auto v_half = [&](int j) {   // V(:,j) = normalised A'u_j - beta_j v_{j-1}; its squared norm to ss[1 + 2 j]
        double* vj = Vb + (int64_t)j * ldv;
        const double* uj = Ub + (int64_t)j * ldu;
        if (j == 0) {
            spmv<double>(c, At, uj, tv, EPI_NONE, 0.0, nullptr, KC_SPMV_B);
            sumsq<double>(c, n, tv, ss + 1);
            div_sqrt_nz<double>(c, n, tv, vj, ss + 1);
        } else {
            PendNorm<double> pb;
            pb.asq = ss + 2 * j;   // beta_{j+1}^2 (1-based: the step's beta)
            spmv<double>(c, At, uj, vj, EPI_SUB, 0.0, vj - ldv, KC_SPMV_B, nullptr, &pb);
            cgs2<double>(c, n, Vb, ldv, j - 1, hsink, false);
            keep_ss(ss + 1 + 2 * j);
        }
    };
    for (int j = 0; j < kmax; ++j) {
        v_half(j);
        PendNorm<double> pa;
        pa.asq = ss + 1 + 2 * j;
        spmv<double>(c, A, Vb + (int64_t)j * ldv, Ub + (int64_t)(j + 1) * ldu, EPI_SUB, 0.0, Ub + (int64_t)j * ldu,
                     KC_SPMV_A, nullptr, &pa);
        cgs2<double>(c, m, Ub, ldu, j, hsink, false);
        keep_ss(ss + 2 + 2 * j);
        read2(ss + 1 + 2 * j, 2, h2);   // the step's one host read-back
        const double a = std::sqrt(h2[0]), bt = std::sqrt(h2[1]);
        // breakdown: alpha or beta <= tol * (the largest seen); not an error
        if (!(a > btol * big)) {
            broke = true;
            break;
        }
        big = std::max(big, a);
        alpha[j] = a;
        beta[j] = bt;
        k = j + 1;
        if (!(bt > btol * big)) {
            broke = true;
            break;
        }
        big = std::max(big, bt);
    }
    if (!broke) {   // one more half step: alpha_{k+1} for the residual estimates
        v_half(k);
        read2(ss + 1 + 2 * k, 1, h2);
        alpha_next = std::sqrt(h2[0]);
    }
    if (steps_done) *steps_done = k;
    if (k == 0) return HGM_OK;

    // ---- B_k = P S Q' on the host ----
    std::vector<double> sg(k), P((size_t)(k + 1) * k), Qm((size_t)k * k);
    dense::bidiag_svd(k, alpha.data(), beta.data(), sg.data(), P.data(), Qm.data());
    const int ns = std::min(nsv, k);
    for (int i = 0; i < ns; ++i) {
        double* pi = &P[(size_t)i * (k + 1)];
        double* qi = &Qm[(size_t)i * k];
        if (pi[0] < 0) {   // u~_i'b >= 0: the sign flips the triplet as a whole
            for (int r = 0; r <= k; ++r) pi[r] = -pi[r];
            for (int r = 0; r < k; ++r) qi[r] = -qi[r];
        }
        sigma[i] = sg[i];
        utb[i] = beta1 * pi[0];
        resid[i] = broke ? 0.0 : alpha_next * std::fabs(pi[k]);
    }

    // ---- VtX = Q(:,1:ns)' (V_k' X): one block pass over V_k ----
    if (nx > 0) {
        const int64_t ldxd = round_up(n, 2);
        double* Xd = c->buf<double>("sv_X", (size_t)ldxd * nx);
        double* tmp = po.trivial() ? nullptr : c->buf<double>("sv_tmp", n);
        for (int r = 0; r < nx; ++r) {
            double* dst = Xd + (size_t)r * ldxd;
            if (po.trivial()) {
                h2d(c, dst, X + (size_t)r * ldx, sizeof(double) * n);
            } else {
                h2d(c, tmp, X + (size_t)r * ldx, sizeof(double) * n);
                pix_permute<double>(c, po, tmp, dst, 0);
            }
        }
        double* Cd = c->buf<double>("sv_C", (size_t)k * nx);
        basis_project(c, n, k, Vb, ldv, nx, Xd, ldxd, Cd);
        std::vector<double> C((size_t)k * nx);
        read2(Cd, k * nx, C.data());
        for (int r = 0; r < nx; ++r)
            for (int i = 0; i < ns; ++i) {
                double s = 0;
                for (int j = 0; j < k; ++j) s += Qm[(size_t)i * k + j] * C[(size_t)r * k + j];
                VtX[(size_t)r * nsv + i] = s;
            }
    }

    // ---- U = U_{k+1} P(:,1:ns), V = V_k Q(:,1:ns): one block pass per 64 columns ----
    auto vectors = [&](double* out, int64_t ldo, int64_t rows, const double* basis, int64_t ldb, int kb,
                       const std::vector<double>& Y, const PixOrder& ord) {
        if (!out) return;
        const int64_t ldw = round_up(rows, 2);
        const int pc = std::min(ns, 64);
        double* Yd = c->buf<double>("sv_Y", (size_t)kb * pc);
        double* W = c->buf<double>("sv_W", (size_t)ldw * pc);
        double* tmp = ord.trivial() ? nullptr : c->buf<double>("sv_tmp", rows);
        for (int c0 = 0; c0 < ns; c0 += 64) {
            const int p = std::min(64, ns - c0);
            h2d(c, Yd, &Y[(size_t)c0 * kb], sizeof(double) * kb * p);
            basis_rotate(c, rows, kb, basis, ldb, p, Yd, kb, W, ldw, nullptr);
            for (int l = 0; l < p; ++l) {
                const double* src = W + (size_t)l * ldw;
                if (!ord.trivial()) {
                    pix_permute<double>(c, ord, src, tmp, 1);
                    src = tmp;
                }
                HGM_HIP(hipMemcpyAsync(out + (size_t)(c0 + l) * ldo, src, sizeof(double) * rows, hipMemcpyDeviceToHost,
                                       c->stream));
                if (!ord.trivial()) stream_sync(c->stream);   // tmp is reused by the next column
            }
            stream_sync(c->stream);
        }
    };
    vectors(U_out, ldu_out, m, Ub, ldu, k + 1, P, PixOrder{});
    vectors(V_out, ldv_out, n, Vb, ldv, k, Qm, po);
    return HGM_OK;
}

}  // namespace hgm
