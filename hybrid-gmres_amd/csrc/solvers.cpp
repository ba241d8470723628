// Solver loops of the reference, driven from the host over the HIP kernels.
//
// Each function follows one reference .m file; the per-line correspondence is
// cited inline.  Vectors live in HBM for the whole solve; per iteration the host
// only receives the new Hessenberg column (k+2 doubles) and a few scalars, and
// sends back the k-vector y of the projected solve.
//
// Multi-GPU (ctx->world > 1): the pixel dimension n is sharded
// (A_g = A(:,P_g), B_g = B(P_g,:)); every `A*v` is followed by an all-reduce of the
// m-vector, every inner product of n-vectors by a scalar all-reduce; m-vectors
// (b, u, the AB-side Krylov basis, A*Q columns) are replicated.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <type_traits>
#include <vector>

#include "internal.h"

namespace hgm {

namespace {

constexpr double EPSD = std::numeric_limits<double>::epsilon();

// 0: the m-space Gram error monitor's side dot x_true'(B*q_k) stays with the MGS sweep instead of
// riding the one pass over B (the A/B build of DESIGN.md §3.5)
#ifndef HGM_FUSED_ZX
#define HGM_FUSED_ZX 1
#endif

// Scalar slots in ctx->dscal.
enum Slot { S_NB = 0, S_NXT = 1, S_BETA = 2, S_RES = 3, S_ERR = 4, S_ALPHA = 5, S_AR = 6, S_FRO = 7,
            S_AUX = 8, S_AUX2 = 9 };

template <typename T>
T* dslot(hgm_ctx* c, int i) {
    return reinterpret_cast<T*>(c->dscal) + i;
}

// y = A x (+epilogue) where the output is an m-vector assembled across ranks.
template <typename T>
void apply_A(hgm_ctx* c, const hgm_mat* A, const T* x, T* y, int epi, T a, const T* z) {
    if (!dist_n(c)) {
        spmv<T>(c, A, x, y, epi, a, z, KC_SPMV_A);
    } else if (epi == EPI_NONE) {
        spmv<T>(c, A, x, y, EPI_NONE, T(0), nullptr, KC_SPMV_A);
        allreduce(c, y, A->rows);
    } else {
        // z may alias y (u = A*v - alpha*u): assemble in scratch, then apply the epilogue
        T* tmp = c->buf<T>("ar_tmp", A->rows + 1);
        spmv<T>(c, A, x, tmp, EPI_NONE, T(0), nullptr, KC_SPMV_A);
        allreduce(c, tmp, A->rows);
        epilogue<T>(c, A->rows, tmp, epi, a, z);
        HGM_HIP(hipMemcpyAsync(y, tmp, sizeof(T) * A->rows, hipMemcpyDeviceToDevice, c->stream));
    }
}

// y = B u (+epilogue): B's rows are this rank's pixels, no exchange.
template <typename T>
void apply_B(hgm_ctx* c, const hgm_mat* B, const T* u, T* y, int epi, T a, const T* z) {
    spmv<T>(c, B, u, y, epi, a, z, KC_SPMV_B);
}

// local sum of squares of an n-vector (+ all-reduce) into slot
template <typename T>
void nsumsq(hgm_ctx* c, int64_t n, const T* v, T* slot) {
    sumsq<T>(c, n, v, slot);
    if (dist_n(c)) allreduce(c, slot, 1);
}
template <typename T>
void nsumsq_diff(hgm_ctx* c, int64_t n, const T* a, const T* b, T* slot) {
    sumsq_diff<T>(c, n, a, b, slot);
    if (dist_n(c)) allreduce(c, slot, 1);
}

template <typename T>
T read1(hgm_ctx* c, const T* dev) {
    T v;
    Reader r(c);
    r.add(&v, dev, sizeof(T));
    r.go();
    return v;
}

// The Golub-Kahan solvers' one-pass plan, agreed over the ranks.  The one-pass path all-reduces
// [A*v_hat | alpha^2] (m + 1 values) per iteration and the two-pass path A*v (m) plus n-space
// norms, so on a communicator every rank must take the same one: each rank plans its own shard
// (a plan can be refused on some shards only, e.g. the centre tile columns of a fan-beam cut),
// the refusals are summed over the ranks, and the pass runs only if no rank refused.
template <typename T>
const FusedPlan* agreed_gk_plan(hgm_ctx* c, const hgm_mat* A, const hgm_mat* At, bool allowed) {
    const FusedPlan* fp = allowed ? fused_ab_plan(c, A, At) : nullptr;
    if (fp && !fused_gk_ok(c, At, fp)) fp = nullptr;
    if (dist_n(c)) {
        double* f = reinterpret_cast<double*>(c->dscal) + 96;
        const double refused = fp ? 0.0 : 1.0;
        h2d(c, f, &refused, sizeof(double));
        allreduce(c, f, 1);
        if (read1<double>(c, f) != 0.0) fp = nullptr;
    }
    c->path_onepass = fp ? 1 : 0;
    return fp;
}

// The one-pass Golub-Kahan step's arguments (internal.h FusedArgs): q = u, the row epilogue
// v_hat = A'*u - beta*ev in place (beta^2 = *easq; ev == nullptr: the start, no epilogue), w = A*v_hat
// into wm and ||v_hat||^2 = alpha^2 into wm[m], where it rides the m-vector all-reduce.
template <typename T>
FusedArgs<T> gk_pass_args(const T* u, T* ev, const T* easq, T* wm, int64_t m) {
    FusedArgs<T> fa;
    fa.q = u;
    fa.ev = ev;
    fa.easq = easq;
    fa.zout = ev;
    fa.w = wm;
    fa.side_sq = true;
    fa.side_out = wm + m;
    return fa;
}

// Iterations enqueued ahead of the host: body(k) for k = 0, 1, ... in batches of `batch`; between
// batches the host reads the device stop slot (stop_slot; nullptr: never), which holds iteration + 1
// of the first stop, 0 while running.  body returns a stop the host itself found (iteration + 1), 0
// to go on.  Returns the stop, 0 when all maxit iterations ran.
template <typename F>
int batched_iterations(hgm_ctx* c, int maxit, int batch, const double* stop_slot, F&& body) {
    int stop = 0;
    for (int k = 0; k < maxit && stop == 0;) {
        const int kend = std::min(maxit, k + batch);
        for (; k < kend && stop == 0; ++k) stop = body(k);
        if (stop_slot && stop == 0) stop = (int)read1<double>(c, stop_slot);
    }
    return stop;
}

// Partial sums over the pixel shards that ride the NEXT iteration's m-vector all-reduce as its
// trailing elements wm[m+1 ..] instead of taking a collective of their own: e, ||x - x_true||^2 into
// errh[k], and d (fp64 only: a float element cannot carry the double sum), ||A'r||^2 into
// monh[2k + 1].  The rotation kernel after that all-reduce copies the sums into iteration k's
// history slots (ScalarCopy); the last iteration's are summed after the loop.
template <typename T>
struct Ridden {
    T* base = nullptr;       // wm + m + 1; nullptr: nothing rides
    int64_t n = 0;           // trailing elements past alpha^2
    T *e = nullptr, *errh = nullptr;
    double *d = nullptr, *monh = nullptr;
    int last = -1;           // the last iteration enqueued
    // the copies into iteration k's slots
    ScalarCopy<T> into(int k) const {
        ScalarCopy<T> cp;
        if (e) {
            cp.src = e;
            cp.dst = errh + k;
        }
        if (d) {
            cp.dsrc = d;
            cp.ddst = monh + 2 * (size_t)k + 1;
        }
        return cp;
    }
    // elements of iteration k's m-vector all-reduce: [A*v_hat | alpha^2 | iteration k-1's sums]
    int64_t count(int64_t m, int k) const { return (base && k > 0) ? m + 1 + n : m + 1; }
};
template <typename T>
Ridden<T> ride_begin(hgm_ctx* c, bool ride, T* wm, int64_t m, T* errh, double* monh) {
    Ridden<T> r;
    if (!ride) return r;
    r.base = wm + m + 1;
    if (errh) r.e = r.base;
    r.errh = errh;
    if constexpr (std::is_same_v<T, double>)
        if (monh) r.d = r.base + 1;
    r.monh = monh;
    r.n = r.d ? 2 : 1;
    HGM_HIP(hipMemsetAsync(r.base, 0, sizeof(T) * r.n, c->stream));
    return r;
}
template <typename T>
void ride_end(hgm_ctx* c, const Ridden<T>& r) {
    if (!r.base || r.last < 0) return;
    allreduce(c, r.base, r.n);
    copy_scalars<T>(c, r.into(r.last));
}

// res (:44) = |phi_bar| / ||b|| of iterations 0..k from the device history of phi_bar
void read_phib(hgm_ctx* c, const double* phib, int maxit, int k, double nb, std::vector<double>& res) {
    std::vector<double> pbh(maxit);
    Reader rh(c);
    rh.add(pbh.data(), phib, sizeof(double) * maxit);
    rh.go();
    for (int i = 0; i < maxit && i <= k; ++i) res[i] = std::fabs(pbh[i]) / nb;
}

// HGM_DEVICE_PTRS: the kernels read b and x_true in place, and the reconstruction's monitors
// (gemv_rows: z = b or x_true) load them as 16-byte element pairs.  Every pointer handed over must
// be 16-byte aligned (hgmres.h); one that is not is refused before anything is enqueued.
static bool device_ptrs(const hgm_opts* o, const double* b_in, const double* xt_in, const double* x_out) {
    if (!(o && (o->flags & HGM_DEVICE_PTRS))) return false;
    for (const double* p : {b_in, xt_in, x_out})
        HGM_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15) == 0, "HGM_DEVICE_PTRS: b, x_true and x must be 16-byte aligned");
    return true;
}

// Input vector hand-over: device pointer (HGM_DEVICE_PTRS) or host buffer.
template <typename T>
const T* stage_in(hgm_ctx* c, const char* name, const double* p, int64_t n, bool dev) {
    if (p == nullptr) return nullptr;
    if (dev && std::is_same<T, double>::value) return reinterpret_cast<const T*>(p);
    T* d = c->buf<T>(name, n > 0 ? n : 1);
    if (std::is_same<T, double>::value) {
        h2d(c, d, p, sizeof(double) * n);
    } else {
        const double* src = p;
        if (!dev) {
            double* tmp = c->buf<double>(std::string(name) + "_f64", n > 0 ? n : 1);
            h2d(c, tmp, p, sizeof(double) * n);
            src = tmp;
        }
        convert<T>(c, n, src, d);
    }
    return d;
}

template <typename T>
void stage_out(hgm_ctx* c, double* out, const T* d, int64_t n, bool dev) {
    if (out == nullptr || n == 0) return;
    if (std::is_same<T, double>::value) {
        if (dev) {
            HGM_HIP(hipMemcpyAsync(out, d, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
            stream_sync(c->stream);
        } else {
            HGM_HIP(hipMemcpyAsync(out, d, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
            stream_sync(c->stream);
        }
    } else {
        double* tmp = dev ? out : c->buf<double>("out_f64", n);
        convert_back<T>(c, n, d, tmp);
        if (!dev) HGM_HIP(hipMemcpyAsync(out, tmp, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        stream_sync(c->stream);
    }
}

// The stored order of the pixel (n) space shared by A's columns and B's (or A''s) rows;
// the ray (m) space is always in the reference order.
PixOrder n_order(hgm_ctx* c, const hgm_mat* A, const hgm_mat* B) {
    HGM_REQUIRE(A->row_order.trivial() && (!B || B->col_order.trivial()),
                "the ray (m) space must be stored in the reference order");
    if (B) HGM_REQUIRE(B->row_order == A->col_order, "A's columns and B's rows must share one pixel order");
    HGM_REQUIRE(A->col_order.trivial() || !dist_n(c), "pixel-sharded solves need the reference pixel order");
    return A->col_order;
}

// n-vector hand-over in the reference order, permuted into / out of the stored order
template <typename T>
const T* stage_in_n(hgm_ctx* c, const char* name, const double* p, int64_t n, bool dev, const PixOrder& o) {
    const T* d = stage_in<T>(c, name, p, n, dev);
    if (d == nullptr || o.trivial()) return d;
    T* q = c->buf<T>(std::string(name) + "_pix", n);
    pix_permute<T>(c, o, d, q, 0);
    return q;
}

template <typename T>
void stage_out_n(hgm_ctx* c, double* out, const T* d, int64_t n, bool dev, const PixOrder& o) {
    if (out == nullptr || n == 0) return;
    if (o.trivial()) {
        stage_out<T>(c, out, d, n, dev);
        return;
    }
    if (dev && std::is_same<T, double>::value) {   // straight into the caller's device buffer
        pix_permute<T>(c, o, d, reinterpret_cast<T*>(out), 1);
        stream_sync(c->stream);
        return;
    }
    T* q = c->buf<T>("out_pix", n);
    pix_permute<T>(c, o, d, q, 1);
    stage_out<T>(c, out, q, n, dev);
}

void check_dims(const hgm_mat* A, const hgm_mat* B) {
    HGM_REQUIRE(A != nullptr, "A is NULL");
    if (B) {
        HGM_REQUIRE(B->rows == A->cols && B->cols == A->rows,
                    "dimension mismatch: B must be size(A') (n x m)");
        HGM_REQUIRE(B->dtype == A->dtype, "A and B must have the same dtype");
    }
}

}  // namespace

// ============================================================================
// Krylov start and plain operator step shared by the Arnoldi-based solvers
// ============================================================================
KrylovBasis krylov_basis(hgm_ctx* c, const char* name, int64_t dim, int cols, bool dist) {
    KrylovBasis kb{nullptr, krylov_ld(c, dim, dist), dim, cols};
    kb.Q = c->buf<double>(name, (size_t)kb.ld * cols);
    if (krylov_padded(c, kb.ld)) HGM_HIP(hipMemsetAsync(kb.Q, 0, sizeof(double) * kb.ld * cols, c->stream));
    return kb;
}

void start_residual(hgm_ctx* c, const hgm_mat* B, const double* b, bool nspace, const KrylovBasis& kb, double* ss) {
    // hybrid_*_rtp.m:7,9 / gcv_function.m:8 / *_bounds.m:11-13: BA: r0 = B*(b - A*0) ; AB: r0 = b - A*(B*0) = b
    if (nspace) apply_B<double>(c, B, b, kb.Q, EPI_NONE, 0.0, nullptr);
    else HGM_HIP(hipMemcpyAsync(kb.Q, b, sizeof(double) * kb.dim, hipMemcpyDeviceToDevice, c->stream));
    if (!ss) return;
    if (nspace) nsumsq<double>(c, kb.dim, kb.Q, ss);
    else sumsq<double>(c, kb.dim, kb.Q, ss);
}

void apply_M(hgm_ctx* c, const hgm_mat* A, const hgm_mat* B, const FusedPlan* fplan, bool nspace, const double* q,
             double* keep, double* out, bool comm) {
    const bool ar = comm && dist_n(c);
    if (nspace) {                                                              // B*(A*q)
        spmv<double>(c, A, q, keep, EPI_NONE, 0.0, nullptr, KC_SPMV_A);
        if (ar) allreduce(c, keep, A->rows);
        spmv<double>(c, B, keep, out, EPI_NONE, 0.0, nullptr, KC_SPMV_B);
        return;
    }
    if (fplan) {                                                               // A*(B*q), one pass over B
        fused_ab(c, B, fplan, q, keep, out);
    } else {
        spmv<double>(c, B, q, keep, EPI_NONE, 0.0, nullptr, KC_SPMV_B);
        spmv<double>(c, A, keep, out, EPI_NONE, 0.0, nullptr, KC_SPMV_A);
    }
    if (ar) allreduce(c, out, A->rows);
}

// ============================================================================
// GMRES family (Arnoldi + projected solve)
// ============================================================================

// Ring polling (single GPU): the host waits for step k by watching the entries of ring
// slot k turn from a NaN sentinel into values instead of an event recorded after the step.
// A recorded event (a marker packet, or a completion signal on the step's last dispatch)
// makes the next kernel wait for an end-of-kernel release: ~4.5 us per step on the main
// stream (rocprofv3 trace).  Every ring entry is written exactly once per
// solve by a system-scope store (st_sys), so a non-sentinel value is final.
constexpr uint64_t RING_SENTINEL = 0x7FF4DEADBEEF0001ull;   // a NaN no kernel produces
// Spin until ring[i] for i in idx are all non-sentinel.  Checks the streams that write them
// (main and, when it is a different one, aux) for errors, and for all going idle with an entry
// never written (a bug), every RING_CHECK_MS so a fault cannot hang.  Not more often: a
// hipStreamQuery on a stream with work queued puts a marker packet behind that work, and the
// kernel queued after the marker then starts ~5.7 us late (round 6: at the 1 ms interval every
// Arnoldi step from the fourth on waited so at C4, profiles/r6_hip_api_trace_gaps.txt).
constexpr int RING_CHECK_MS = 200;
static void ring_wait(hgm_ctx* c, const double* ring, const std::vector<size_t>& idx, hipStream_t aux = nullptr) {
    const volatile uint64_t* r = reinterpret_cast<const volatile uint64_t*>(ring);
    const auto t0 = std::chrono::steady_clock::now();
    auto last = t0;
    bool idle_seen = false;
    HostPause pause;
    for (;;) {
        bool all = true;
        for (size_t i : idx)
            if (r[i] == RING_SENTINEL) {
                all = false;
                break;
            }
        if (all) break;
        pause();
        const auto now = std::chrono::steady_clock::now();
        if (now - last > std::chrono::milliseconds(RING_CHECK_MS)) {
            last = now;
            hipError_t q = hipStreamQuery(c->stream);
            if (q != hipSuccess && q != hipErrorNotReady) HGM_HIP(q);
            if (aux && aux != c->stream && q == hipSuccess) {   // idle only when both streams are
                q = hipStreamQuery(aux);
                if (q != hipSuccess && q != hipErrorNotReady) HGM_HIP(q);
            }
            if (q == hipSuccess) {
                if (idle_seen) throw Error{HGM_E_HIP, "ring poll: stream idle with a ring entry never written"};
                idle_seen = true;   // one more round: the last stores may still be in flight
            }
        }
    }
    if (c->host_stats) {
        c->wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
}

int gmres_family(hgm_ctx* c, const GmresSpec& sp, const hgm_opts* o, const hgm_mat* A, const hgm_mat* B,
                 const double* b_in, const double* xt_in, double tol, int maxit, double lambda, double* x_out,
                 double* err_out, double* res_out, int* niters, KrylovBasis* basis_out) {
    check_dims(A, B);
    HGM_REQUIRE(B != nullptr, "B is NULL");
    const PixOrder po = n_order(c, A, B);
    HGM_REQUIRE(b_in != nullptr && xt_in != nullptr, "b and x_true are required");
    HGM_REQUIRE(A->dtype == HGM_F64, "GMRES family is fp64 (the reference's precision)");
    const auto t_start = std::chrono::steady_clock::now();
    const double wait0 = c->wait_s;
    const long waits0 = c->waits;
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    c->path_mon.clear();
    const bool dev = device_ptrs(o, b_in, xt_in, x_out);
    const int orth = o ? o->orth : HGM_MGS;
    const int64_t m = A->rows, n = A->cols;
    const bool nspace = sp.side == HGM_SIDE_BA;
    const int64_t dim = nspace ? n : m;
    const bool dist = nspace && dist_n(c);
    // parity mode (HGM_OPT_PARITY): the reference's own sequence of operations in
    // fixed summation orders; every fused or reformulated monitor below is switched off
    const bool parity = c->num.parity;
    HGM_REQUIRE(!parity || (!dist_n(c) && po.trivial()), "parity mode: single rank, reference pixel order");
    hipStream_t st = c->stream;

    const KrylovBasis kb = krylov_basis(c, "Q", dim, maxit + 1, dist);
    if (basis_out) *basis_out = kb;
    double* Q = kb.Q;
    const int64_t ldq = kb.ld;
    double* x = c->buf<double>("x", n > 0 ? n : 1);
    double* t = c->buf<double>("t_m", m > 0 ? m : 1);        // m-vector scratch (A*q, residual)
    double* tn = c->buf<double>("t_n", n > 0 ? n : 1);       // n-vector scratch (AB side: B*q)
    double* z = c->buf<double>("z_m", m > 0 ? m : 1);        // AB side: z = Q*y
    double* tr = c->buf<double>("t_res", m > 0 ? m : 1);     // m-vector of the residual monitor (aux stream)
    const int64_t ldaq = round_up(m > 0 ? m : 1, 64);
    // n-space side: keep the operator's products A*Q(:,j) (the RTP Gram matrix needs them,
    // and the residual monitor b - A*x = b - (A*Q) y reuses them instead of another SpMV)
    const bool reuse = !(o && (o->flags & HGM_EXPLICIT_RESIDUAL)) && !parity;
    const bool aq_res = nspace && reuse;
    double* AQ = (sp.proj == PROJ_ABRTP || aq_res) ? c->buf<double>("AQ", (size_t)ldaq * maxit) : nullptr;
    // m-space side: keep B*Q(:,j) and A*(B*Q(:,j)) (the latter is the new Arnoldi vector
    // before orthogonalisation), so x = B*(Q y) = (B*Q) y and b - A*x = b - (A*B*Q) y are
    // GEMVs over k kept columns instead of two SpMVs per iteration (*_bounds.m:37-40)
    const bool bq_res = !nspace && reuse;
    const int64_t ldbq = round_up(n > 0 ? n : 1, 64);
    double* BQ = bq_res ? c->buf<double>("BQ", (size_t)ldbq * maxit) : nullptr;
    double* ABQ = bq_res ? c->buf<double>("ABQ", (size_t)ldaq * maxit) : nullptr;
    // Per-iteration exchange ring in pinned host memory: slot k holds
    // [H(:,k) | Gram column k, AQk'b] (LH doubles), the monitors [res^2, err^2] of
    // iteration k, and the projected solution y_k.  Single GPU: the kernels write the
    // slots in place and read y from it (zero-copy, no copy kernels).  Multi-GPU m-space side
    // (the sharded AB-GMRES of configs[3]): the same, since the m-space sweep is replicated and
    // every ring entry is written after its all-reduce (a sum that is all-reduced is formed in a
    // device slot, all-reduced there and copied into the ring by copy_sys).  Multi-GPU n-space
    // side: the all-reduced sweep scalars live in a device mirror and each slot is copied out once.
    const size_t LH = 2 * (size_t)(maxit + 2);
    const size_t offM = (size_t)maxit * LH, offY = offM + 2 * (size_t)maxit;
    const size_t offS = offY + (size_t)maxit * maxit;   // [beta, ||b||^2, ||x_true||^2] (polling)
    const bool zc = !dist_n(c) || !nspace;
    // Gram error monitor: step k's MGS sweep appends [Q(:,k)'Q(:,0:k-1),
    // Q(:,k)'Q(:,k), Q(:,k)'x_true] to the ring (LQ doubles) and the host evaluates
    // ||Q y_k - x_true||^2 from them, so an iteration's reconstruction reads only the kept A*Q.
    const bool gem_ok = zc && c->num.ring_poll && orth == HGM_MGS && mgs_gram_ok(c, ldq, maxit, dist) &&
                        c->num.gram_err;
    const bool gem_n = aq_res && gem_ok;
    // m-space side (AB-GMRES, x = (B*Q) y = Z y): when B is A' value for value (a device
    // transpose), Z'Z = Q'(A*B*Q) are the sweep's own dots Q'w_k = (I + L) H(0:k,k) (one-reduction
    // form, L the strictly lower Q'Q), and Z'x_true = x_true'(B*q_k) is one dot per step riding on
    // the sweep as a side job, so an iteration's reconstruction reads no n-vector: the kept B*Q
    // columns are combined once, at the end (C4: the 0.3 ms GEMV per iteration)
    const bool pair_t = B && (B->transpose_of == A->uid || A->transpose_of == B->uid);
    // (multi-GPU too: the m-space sweep is replicated, the side dot is all-reduced and the
    // Gram row published with the H column; a shard pair A_g = B_g' qualifies)
    const bool gem_ab = bq_res && orth == HGM_MGS && mgs_gram_ok(c, ldq, maxit, dist) && c->num.gram_err &&
                        (zc ? c->num.ring_poll : true) && sp.proj != PROJ_ABRTP && pair_t;
    const bool gem = gem_n || gem_ab;
    const double gem_min = c->num.gram_err_min;
    const size_t LQ = (size_t)maxit + 2, offQG = offS + 4;
    const size_t ring_n = offQG + (gem ? (size_t)maxit * LQ : 0);
    // single GPU: reconstructions run on the auxiliary stream, concurrently with the
    // Arnoldi steps (multi-GPU keeps one stream: the communicator's collectives must be
    // issued in one order).  For large n the concurrent GEMV over the kept columns evicts
    // the SpMVs' L2-resident x-slices and costs the SpMVs more than it hides, so it is
    // serialised behind the steps (HGM_RECON_SERIAL=0/1 overrides).
    // (with the Gram error monitor the per-iteration reconstruction reads only the kept A*Q,
    // so it stays on the aux stream at any n: C3 1,376 vs 1,368 iters/s serialised)
    bool recon_serial = !gem && (int64_t)n >= c->num.recon_serial_n;
    if (c->num.recon_serial >= 0) recon_serial = c->num.recon_serial != 0;
    // (a communicator's solve keeps one stream whatever the ring)
    // On a communicator the m-space solve's residual-only reconstructions (gem_ab: the kept A*B*Q
    // columns and b are replicated, so no collective runs in them) go to the auxiliary stream as
    // well; a reconstruction that forms x all-reduces its error and stays on the step stream, so
    // the communicator's collectives keep one stream and one order on every rank.
    // Scratch invariant: reconstructions on the auxiliary stream and the x-forming ones
    // on the step stream share the recon_parts / recon_noerr scratch buffers.  That is safe only
    // because the host waits for reconstruction k's ring slots (ring_wait on both streams) before
    // it enqueues reconstruction k+1 on either stream, so two reconstructions never run at once.
    const bool rs_aux_dist = dist_n(c) && gem_ab && !recon_serial && zc;
    hipStream_t rs_stream = (zc && !recon_serial && (!dist_n(c) || rs_aux_dist)) ? aux_stream(c) : st;
    if (rs_stream != st) stream_sync(rs_stream);
    pinned_ring(c, sizeof(double) * ring_n);
    const double* hr = c->hring;
    const bool poll = zc && c->num.ring_poll && !parity;
    // the reconstruction's pipeline event: not needed when the host polls the ring and the
    // reconstruction runs on the step stream (an event there is a bubble between two kernels)
    const bool pipe_ev = !(poll && rs_stream == st);
    if (zc) {
        // the kernels store into the mapped ring with system-scope stores, and the pipeline
        // events carry no system-scope release, so a store may land after its kernel's event
        // has completed: the host spins on a sentinel for every entry it reads, with or without
        // polling (an event wait then only saves the spinning)
        uint64_t* r = reinterpret_cast<uint64_t*>(c->hring);
        for (size_t i = 0; i < (size_t)maxit * LH; ++i) r[i] = RING_SENTINEL;
        for (size_t i = offM; i < offM + 2 * (size_t)maxit; ++i) r[i] = RING_SENTINEL;
        if (poll)
            for (size_t i = offS; i < offS + 3; ++i) r[i] = RING_SENTINEL;
        for (size_t i = offQG; i < ring_n; ++i) r[i] = RING_SENTINEL;
    }
    double* dr = zc ? c->hring_dev : c->buf<double>("ring_dev", ring_n);
    auto publish = [&](size_t off, size_t cnt) {
        if (!zc)
            HGM_HIP(hipMemcpyAsync(c->hring + off, dr + off, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
    };
    // inputs staged after the ring reset (its stream sync then finds the GPU idle)
    const double* b = stage_in<double>(c, "in_b", b_in, m, dev);
    const double* xt = stage_in_n<double>(c, "in_xt", xt_in, n, dev, po);
    fill<double>(c, n, x, 0.0);

    std::vector<double> H((size_t)(maxit + 1) * maxit, 0.0);
    std::vector<double> err(maxit, 0.0), res(maxit, 0.0);
    auto Hh = [&](int i, int j) -> double& { return H[(size_t)j * (maxit + 1) + i]; };

    // ||b|| (m, replicated) and ||x_true|| (n, sharded) — MATLAB recomputes them every
    // iteration (hybrid_*_rtp.m:32-33); the values are loop-invariant.
    double nb = 0, nxt = 0, beta = 0, xt2 = 0;
    double* q0 = Q;
    // (a communicator all-reduces the x_true norm over the pixel shards: the second branch, whatever
    // stream the reconstructions use)
    if (poll && dev && rs_stream != st && !dist_n(c)) {
        // no host round trip before the first step: the norms land in the ring (read at
        // iteration 0) and r0 is divided on the device.  With device inputs the two norms
        // run on the aux stream, beside B*b (x_true in the caller's order: same norm).
        StreamScope scope(c, rs_stream, "aux:");
        sumsq<double>(c, m, b, dr + offS + 1);
        sumsq<double>(c, n, xt_in, dr + offS + 2);   // ||x_true - 0||^2
    } else if (poll && dist_n(c)) {
        sumsq<double>(c, m, b, dr + offS + 1);                    // (m: replicated)
        sumsq<double>(c, n, xt, dslot<double>(c, S_NXT));              // ||x_true - 0||^2 over the pixel shards
        allreduce(c, dslot<double>(c, S_NXT), 1);
        copy_sys(c, dslot<double>(c, S_NXT), dr + offS + 2);
    } else if (poll) {
        sumsq<double>(c, m, b, dr + offS + 1);
        sumsq<double>(c, n, xt, dr + offS + 2);                   // ||x_true - 0||^2
    } else {
        sumsq<double>(c, m, b, dslot<double>(c, S_NB));
        nsumsq_diff<double>(c, n, xt, x, dslot<double>(c, S_NXT));   // ||x_true - 0||^2
    }
    start_residual(c, B, b, nspace, kb, poll ? nullptr : dslot<double>(c, S_BETA));   // r0
    if (poll) {
        normalize_to<double>(c, dim, q0, dr + offS);           // :10,:13  beta = norm(r0); Q(:,1) = r0 / beta
    } else {
        read_scalars(c, 0, 3);
        nb = std::sqrt(c->hscal[S_NB]);
        nxt = std::sqrt(c->hscal[S_NXT]);
        xt2 = c->hscal[S_NXT];
        beta = std::sqrt(c->hscal[S_BETA]);               // :10  beta = norm(r0)
        div_scalar<double>(c, dim, q0, q0, beta);           // :13  Q(:,1) = r0 / beta
    }

    bool x_assigned = sp.x_preassigned;
    int k = 0;
    std::vector<double> y, M;
    std::vector<double> G((size_t)maxit * maxit, 0.0), cvec(maxit, 0.0);
    // Gram error monitor: Q'Q, Q'x_true and the errors it produced (-1: formed explicitly)
    // (m-space: the Gram of Z = B*Q, from H and the strictly lower Q'Q in SQ)
    std::vector<double> GQ(gem ? (size_t)maxit * maxit : 0), cq(maxit, 0.0), gerr(maxit, -1.0);
    std::vector<double> SQ(gem_ab ? (size_t)maxit * maxit : 0);
    // Pending normalisation (one-reduction MGS): step k leaves v_{k+1} = Q(:,k+1)
    // undivided and step k+1 applies q = v / H(k+1,k) where it reads it — n-space (single GPU):
    // A: (A*v)/h, which also publishes h = H(k+1,k); B: B*(A*q) + lambda*q; m-space: the one pass
    // over B stages q = v/h and publishes h; the MGS dots kernel writes q back over v — so the
    // sweep needs no scale pass.  Step k's event is then
    // recorded at the end of step k+1.  HGM_OPT_PEND_NORM = 0 keeps the scale pass.
    // m-space side with B = A' value for value: B*q and A*(B*q) in one pass over B (fused.hip)
    const FusedPlan* fplan = nspace ? nullptr : fused_ab_plan(c, A, B);
    // (m-space, round 6: the one pass over B applies q = v / h as it stages q, so the m-space sweep
    // needs no scale pass either; the m-vectors are replicated, so this holds on a communicator too,
    // every rank forming the same h from the same replicated partials)
    // (m-space only with HGM_OPT_PEND_NORM = 2: the pass's staging then waits for the division, which
    // measured ~1.4 % slower at C4 than the scale pass it replaces)
    const bool pn_ok = !dist && orth == HGM_MGS && c->num.pend_norm >= 1 && !parity &&
                       (nspace ? spmv_pn_ok(A, EPI_DIVH) && spmv_pn_ok(B, EPI_ADDQ)
                               : c->num.pend_norm == 2 && fplan != nullptr && !krylov_padded(c, ldq));
    PendNorm<double> pend;                                  // np > 0: Q(:,next step) awaits its division
    double* pn_h = c->buf<double>("pn_h", 2);
    // Enqueue Arnoldi step kq: operator application + orthogonalisation (+ Gram column).
    auto enqueue_step = [&](int kq) {
        bool zx_fused = false;                            // x_true'(B*q_k) formed by the fused pass
        bool zx_rode = false;                             // ... and summed over the ranks with A*(B*q_k)
        double* qk = Q + (int64_t)kq * ldq;
        double* v = Q + (int64_t)(kq + 1) * ldq;
        const bool pending_in = pend.np > 0;
        // ---- operator (hybrid_*_rtp.m:19 ; *_bounds.m:25) ----
        if (nspace && pending_in) {
            double* Aq = AQ ? AQ + (int64_t)kq * ldaq : t;
            PendNorm<double> pa = pend;
            pa.hdev = pn_h;
            pa.hring = dr + (size_t)(kq - 1) * LH + kq;    // H(kq, kq-1) of step kq-1
            spmv<double>(c, A, qk, Aq, EPI_DIVH, 0.0, nullptr, KC_SPMV_A, nullptr, &pa);   // A*q = (A*v)/h
            PendNorm<double> pb;
            pb.hdev = pn_h;
            // B*(A*q) + lambda*q with q = v/h (lambda = 0: B*(A*q) + 0*q); the MGS dots kernel
            // writes q back over v
            spmv<double>(c, B, Aq, v, EPI_ADDQ, sp.lambda_in_op ? lambda : 0.0, qk, KC_SPMV_B, nullptr, &pb);
        } else if (nspace) {
            double* Aq = AQ ? AQ + (int64_t)kq * ldaq : t;
            if (sp.lambda_in_op) {
                apply_A<double>(c, A, qk, Aq, EPI_NONE, 0.0, nullptr);
                apply_B<double>(c, B, Aq, v, EPI_ADD, lambda, qk);                  // B*(A*v) + lambda*v
            } else {
                apply_M(c, A, B, nullptr, true, qk, Aq, v);                         // B*(A*v)
            }
        } else {
            double* Bq = BQ ? BQ + (int64_t)kq * ldbq : tn;
            // A*(B*Q(:,k)) lands in its kept column (MGS reads it from there and writes the
            // orthogonalised vector to Q(:,k+1), no copy), or in Q(:,k+1) for CGS2
            double* w = (ABQ && orth != HGM_CGS2) ? ABQ + (int64_t)kq * ldaq : v;
            if (fplan) {
                // both in one pass over B; with the m-space Gram error monitor the pass also forms
                // the side dot x_true'(B*Q(:,k)) (else the MGS sweep's extra workgroups do)
                const bool zxf = HGM_FUSED_ZX && gem_ab;
                // (on a communicator the rank-local dot goes to a device slot, all-reduced below)
                double* zx_dst =
                    zxf ? (dist_n(c) ? dslot<double>(c, S_AUX2) : dr + offQG + (size_t)kq * LQ + kq + 2) : nullptr;
                // on a communicator the side dot rides the m-vector all-reduce as its element m
                // (when the column's stride leaves room past m): one collective per step, not two
                const int64_t wld = (ABQ && orth != HGM_CGS2) ? ldaq : ldq;
                const bool ride = zxf && dist_n(c) && wld > m;
                PendNorm<double> pq;                                // q_k = v_k / H(k,k-1) as the pass stages it
                if (pending_in) {
                    pq = pend;
                    pq.hdev = pn_h;
                    pq.hring = dr + (size_t)(kq - 1) * LH + kq;  // H(kq, kq-1) of step kq-1
                }
                zx_fused = fused_ab(c, B, fplan, qk, Bq, w, zxf ? xt : nullptr, ride ? w + m : zx_dst,
                                    pending_in ? &pq : nullptr);
                zx_rode = ride && zx_fused;
                if (dist_n(c)) allreduce(c, w, zx_rode ? m + 1 : m);             // (as apply_A)
                // (the all-reduced side dot goes into the ring with the MGS sweep below)
            } else {
                apply_M(c, A, B, nullptr, false, qk, Bq, w);                        // B*Q(:,k), A*(B*Q(:,k))
            }
            if (ABQ && orth == HGM_CGS2)
                HGM_HIP(hipMemcpyAsync(ABQ + (int64_t)kq * ldaq, v, sizeof(double) * m, hipMemcpyDeviceToDevice,
                                       c->stream));
        }
        // ---- orthogonalisation (hybrid_*_rtp.m:20-26) ----
        double* Hcol = dr + (size_t)kq * LH;                  // -> host H(:,k)
        // column k of AQk'*AQk and AQk'*b (hybrid_ab_gmres_rtp.m:31-32); A*Q(:,j) was
        // computed inside M_reg_op(Q(:,j)) at :19 — the same deterministic SpMV.  With MGS
        // it runs as extra workgroups of the sweep's first two passes.
        MdotJob<double> gram;
        if (sp.proj == PROJ_ABRTP) {
            gram.n = m;
            gram.ncols = kq + 1;
            gram.Q = AQ;
            gram.ldq = ldaq;
            gram.w = AQ + (int64_t)kq * ldaq;
            gram.e = b;                                   // + b'*AQ(:,k)
            gram.out = Hcol + (maxit + 2);
        }
        const MdotJob<double>* side = sp.proj == PROJ_ABRTP ? &gram : nullptr;
        if (orth == HGM_CGS2) {
            cgs2<double>(c, dim, Q, ldq, kq, Hcol, dist);
            if (side) multidot<double>(c, m, gram.ncols, AQ, ldaq, gram.w, gram.out, b);
        } else {
            PendNorm<double>* defer = (pn_ok && kq + 1 < maxit) ? &pend : nullptr;
            if (!defer) pend.np = 0;
            MdotJob<double> zx;                                // gem_ab: x_true'(B*q_k) -> row entry k+2
            double* zx_ring = dr + offQG + (size_t)kq * LQ + kq + 2;
            if (gem_ab) {
                zx.n = n;
                zx.w = BQ + (int64_t)kq * ldbq;
                zx.e = xt;
                zx.out = dist_n(c) ? dslot<double>(c, S_AUX2) : zx_ring;   // (the fused pass's zx_dst too)
            }
            // the Gram row's extra dot: x_true (n-space) or b (m-space, unused: the row is for L)
            const double* cps = nullptr;
            double* cpd = nullptr;
            if (zx_rode) {
                cps = ABQ ? ABQ + (int64_t)kq * ldaq + m : v + m;
                cpd = dr + offQG + (size_t)kq * LQ + kq + 2;
            }
            mgs<double>(c, dim, Q, ldq, kq, Hcol, dist, (!nspace && ABQ) ? ABQ + (int64_t)kq * ldaq : nullptr,
                        gem_ab ? (zx_fused ? nullptr : &zx) : side, defer, pending_in ? pn_h : nullptr,
                        gem ? (gem_n ? xt : b) : nullptr, gem ? dr + offQG + (size_t)kq * LQ : nullptr, cps, cpd);
            if (gem_ab && dist_n(c) && !zx_rode) {        // x_true'(B*q_k) over the pixel shards
                allreduce(c, zx.out, 1);
                copy_sys(c, zx.out, zx_ring);
            }
        }
        // Step kq-1's column is complete (H(kq,kq-1) came from this step's A product).  The
        // event goes at the end of the step: a marker between two kernels costs a bubble.
        if (poll) return;                                 // the host polls the ring instead
        if (pending_in) {
            publish((size_t)(kq - 1) * LH, LH);
            if (gem_ab) publish(offQG + (size_t)(kq - 1) * LQ, (size_t)kq + 2);   // its Gram row
            step_record(c, kq - 1);
        }
        if (pend.np == 0) {                               // else: recorded at the end of step kq+1
            publish((size_t)kq * LH, LH);
            if (gem_ab) publish(offQG + (size_t)kq * LQ, (size_t)kq + 3);   // the Gram row (m-space)
            step_record(c, kq);
        }
    };
    // Reconstruction + monitors of iteration kq from y_kq (in the ring) on the auxiliary
    // stream, then the event the host waits on.  Everything it reads (Q(:,0..kq), y_kq)
    // is complete when it is enqueued (the host has seen step kq finish), so it needs no
    // stream dependency; it writes only x, its own scratch and ring slot kq.
    int x_pending = -1;   // the last reconstruction, when it left x unformed (Gram error monitor)
    auto enqueue_recon = [&](int kq, bool want_x) {
        StreamScope scope(c, (rs_aux_dist && want_x) ? st : rs_stream, (rs_aux_dist && want_x) ? "" : "aux:");
        const int kk = kq + 1;
        const double* yk = c->hring_dev + offY + (size_t)kq * maxit;
        double* rslot = dr + offM + 2 * (size_t)kq;
        double* eslot = rslot + 1;
        // an error sum over the pixel shards is all-reduced in a device slot, then copied into the
        // (host-mapped) ring
        double* eloc = (dist_n(c) && zc) ? dslot<double>(c, S_ERR) : eslot;
        auto err_done = [&](bool reduce) {
            if (reduce && dist_n(c)) allreduce(c, eloc, 1);
            if (eloc != eslot) copy_sys(c, eloc, eslot);
        };
        // ---- reconstruction (hybrid_*_rtp.m:30/33 ; *_bounds.m:37-38) ----
        if (aq_res) {
            // x = Q(:,1:k)*yk with ||x - x_true||^2 (:33/:36) and ||b - A*x||^2 (:32/:35)
            // evaluated as ||b - (A*Q(:,1:k))*yk||^2, all in one launch (+ finalize)
            // (want_x false: the Gram error monitor has the error, x is formed at the end)
            recon<double>(c, n, kk, Q, ldq, yk, want_x ? x : nullptr, xt, eslot, m, AQ, ldaq, b, rslot);
            x_pending = want_x ? -1 : kq;
            if (dist_n(c)) allreduce(c, eslot, 1);
            publish(offM + 2 * (size_t)kq, 2);
            if (pipe_ev) pipe_record(c);
            return;
        }
        if (bq_res) {
            // xk = B*(Q(:,1:k)*yk) = (B*Q(:,1:k))*yk with ||xk - x_true||^2, and
            // ||b - A*xk||^2 = ||b - (A*B*Q(:,1:k))*yk||^2 (*_bounds.m:37-40), one launch
            // (want_x false: the m-space Gram error monitor has the error, x is formed at the end)
            recon<double>(c, n, kk, BQ, ldbq, yk, want_x ? x : nullptr, xt, eloc, m, ABQ, ldaq, b, rslot);
            x_pending = want_x ? -1 : kq;
            if (want_x) err_done(true);
            publish(offM + 2 * (size_t)kq, 2);
            if (pipe_ev) pipe_record(c);
            return;
        }
        if (nspace) {
            // x = Q(:,1:k)*yk, fused with the error monitor ||x - x_true||^2 (:33 / :36)
            gemv_err<double>(c, n, kk, Q, ldq, yk, x, xt, eslot);
            if (dist_n(c)) allreduce(c, eslot, 1);
        } else {
            gemv<double>(c, m, kk, Q, ldq, yk, z, 0);                 // zk = Q(:,1:k)*yk
            apply_B<double>(c, B, z, x, EPI_NONE, 0.0, nullptr);     // xk = B*zk
            sumsq_diff<double>(c, n, x, xt, eloc);
            err_done(true);
        }
        // ---- monitors (hybrid_*_rtp.m:32-33 / :35-36): norm(b - A*x) ----
        if (!dist_n(c)) {
            spmv<double>(c, A, x, tr, EPI_RSUB, 0.0, b, KC_SPMV_A, rslot);   // sum of squares fused
        } else {
            apply_A<double>(c, A, x, tr, EPI_RSUB, 0.0, b);
            sumsq<double>(c, m, tr, rslot);
        }
        publish(offM + 2 * (size_t)kq, 2);
        if (pipe_ev) pipe_record(c);
    };
    // Software pipeline over two streams, L = HGM_OPT_PIPE_DEPTH:
    //     main: S0 S1 S2 S3 ...          (S_k: Arnoldi step k -> H(:,k), Q(:,k+1))
    //     aux :       R0 R1 R2 ...       (R_k: x = Q y_k, monitors of iteration k)
    // At iteration k the host waits for S_k and R_{k-1}, solves for y_k, enqueues R_k
    // and then S_{k+L+1}; the GPU meanwhile runs S_{k+1..k+L} and overlaps R_k with
    // them, so it never waits for the host.  When `residual_norm(k) <= tol` stops the loop the
    // speculative steps are discarded: they write only Q(:,>k+1), AQ(:,>k), their own
    // ring slots and scratch — never x or a history — so every output equals the
    // reference's.  (Multi-GPU: both sequences share one stream, same semantics.)
    const int L = c->num.pipe_depth;                     // speculative steps in flight
    for (int j = 0; j <= L && j < maxit; ++j) enqueue_step(j);
    // the mapped-ring entries of step kq (H column, Gram column, Gram error row)
    auto wait_step = [&](int kq) {
        std::vector<size_t> idx;
        for (int i = 0; i < kq + 2; ++i) idx.push_back((size_t)kq * LH + i);
        if (sp.proj == PROJ_ABRTP)
            for (int i = 0; i < kq + 2; ++i) idx.push_back((size_t)kq * LH + (maxit + 2) + i);
        if (gem)
            for (int i = 0; i < kq + 2; ++i) idx.push_back(offQG + (size_t)kq * LQ + i);
        if (gem_ab) idx.push_back(offQG + (size_t)kq * LQ + kq + 2);
        ring_wait(c, hr, idx);
    };
    // the monitors of reconstruction R_kq (the error slot is not written when the Gram error
    // monitor supplied the error)
    auto wait_mon = [&](int kq) {
        if (!zc) return;
        std::vector<size_t> idx{offM + 2 * (size_t)kq};
        if (gerr[kq] < 0) idx.push_back(offM + 2 * (size_t)kq + 1);
        ring_wait(c, hr, idx, rs_stream);
    };
    bool done = false;
    for (k = 0; k < maxit; ++k) {
        if (k >= 1) {                                    // R_{k-1}
            if (pipe_ev) pipe_wait(c);
            wait_mon(k - 1);
        }
        if (poll) {
            // S_k: H(0:k+1,k) (+ Gram column k).  H(k+1,k) is written by a kernel that starts
            // after every kernel of step k has finished (the scale pass of step k, or with the
            // pending normalisation the A product of step k+1), so once it is visible Q(:,0:k)
            // and the kept products of step k, which R_k reads, are complete.
            wait_step(k);
            if (k == 0) {                                // the setup norms (written before step 0;
                                                         // with device inputs partly on the aux stream)
                ring_wait(c, hr, {offS, offS + 1, offS + 2}, rs_stream);
                beta = hr[offS];
                nb = std::sqrt(hr[offS + 1]);
                nxt = std::sqrt(hr[offS + 2]);
                xt2 = hr[offS + 2];
            }
        } else {
            step_wait(c, k);                             // S_k: H(:,k) (+ Gram column k)
            if (zc) wait_step(k);
        }
        if (k >= 1) {
            const double* mk = hr + offM + 2 * (size_t)(k - 1);
            res[k - 1] = std::sqrt(mk[0]) / nb;
            err[k - 1] = gerr[k - 1] >= 0 ? gerr[k - 1] : std::sqrt(mk[1]) / nxt;
            if (res[k - 1] <= tol) {                     // :35 / :38 / *_bounds :79-83
                k = k - 1;
                done = true;
                break;
            }
        }
        const double* hk = hr + (size_t)k * LH;
        for (int i = 0; i < k + 2; ++i) Hh(i, k) = hk[i];
        if (sp.proj == PROJ_ABRTP) {
            for (int i = 0; i <= k; ++i) G[(size_t)k * maxit + i] = hk[(maxit + 2) + i];
            cvec[k] = hk[(maxit + 2) + k + 1];
        }
        if (gem_n) {
            const double* gk = hr + offQG + (size_t)k * LQ;
            for (int i = 0; i < k; ++i) GQ[(size_t)k * maxit + i] = GQ[(size_t)i * maxit + k] = gk[i];
            GQ[(size_t)k * maxit + k] = gk[k];
            cq[k] = gk[k + 1];
        } else if (gem_ab) {
            // z_j'z_k = q_j'(A*B*q_k) = H(j,k) + sum_{i<j} (q_j'q_i) H(i,k): the sweep solved
            // (I + L) h = Q'w_k for h = H(0:k,k), so this is its right-hand side again
            const double* gk = hr + offQG + (size_t)k * LQ;
            for (int i = 0; i < k; ++i) SQ[(size_t)k * maxit + i] = gk[i];
            for (int j = 0; j <= k; ++j) {
                long double g = Hh(j, k);
                for (int i = 0; i < j; ++i) g += (long double)SQ[(size_t)j * maxit + i] * Hh(i, k);
                GQ[(size_t)k * maxit + j] = GQ[(size_t)j * maxit + k] = (double)g;
            }
            cq[k] = gk[k + 2];
        }
        if (Hh(k + 1, k) == 0) {                         // :25  if H(k+1,k) == 0, break
            done = true;
            break;
        }
        const int kk = k + 1;                            // MATLAB k
        y.assign(kk, 0.0);
        if (sp.proj == PROJ_LS) {
            dense::proj_ls(H.data(), maxit + 1, kk, beta, y.data());
        } else if (sp.proj == PROJ_PTR) {
            M.assign((size_t)kk * kk, 0.0);
            dense::normal_matrix(H.data(), maxit + 1, kk, M.data());
            dense::proj_ptr(M.data(), H.data(), maxit + 1, kk, beta, lambda, y.data());
        } else {
            dense::proj_gram(G.data(), maxit, cvec.data(), kk, lambda, y.data());
        }
        std::memcpy(c->hring + offY + (size_t)k * maxit, y.data(), sizeof(double) * kk);
        bool want_x = true;
        // (the last iteration's reconstruction forms x anyway: there the GEMV carries the error)
        if (gem && k + 1 < maxit) {
            // ||Q y - x_true||^2 = x_true'x_true - 2 y'(Q'x_true) + y'(Q'Q) y (hybrid_*_rtp.m:33/:36
            // with x = Q y), used when it is at least gem_min ||x_true||^2 (the cancellation then
            // costs at most a factor 1/gem_min of the terms' rounding)
            long double e2 = xt2;
            for (int i = 0; i < kk; ++i) {
                long double gy = 0;
                for (int j = 0; j < kk; ++j) gy += (long double)GQ[(size_t)i * maxit + j] * y[j];
                e2 += (long double)y[i] * (gy - 2.0L * cq[i]);
            }
            if (xt2 > 0 && e2 >= (long double)gem_min * xt2) {
                gerr[k] = std::sqrt((double)e2) / nxt;
                want_x = false;
            }
        }
        c->path_mon.push_back(want_x ? 0 : 1);
        enqueue_recon(k, want_x);
        x_assigned = true;
        if (k + L + 1 < maxit) enqueue_step(k + L + 1);  // speculative, see above
    }
    if (x_pending >= 0) {
        // the last reconstruction left x unformed (Gram error monitor): x = Q(:,0:k) y_k
        // behind it, on the same stream
        StreamScope scope(c, rs_stream, "aux:");
        const double* yk = c->hring_dev + offY + (size_t)x_pending * maxit;
        if (nspace) gemv<double>(c, n, x_pending + 1, Q, ldq, yk, x, 0);
        else gemv<double>(c, n, x_pending + 1, BQ, ldbq, yk, x, 0);          // x = (B*Q) y
        x_pending = -1;
    }
    bool staged = false;
    if (!done) {
        // all maxit iterations ran: the last monitors are still outstanding.  With the
        // reconstruction on the aux stream, x is staged out behind it there (one sync, no
        // host wake-up in between).
        // (x_out == NULL: nothing to stage, so wait for the last monitors explicitly)
        // (a communicator's last reconstruction formed x on the step stream: staged out there below)
        if (rs_stream != st && !rs_aux_dist && x_assigned && x_out != nullptr) {
            StreamScope scope(c, rs_stream, "aux:");
            stage_out_n<double>(c, x_out, x, n, dev, po);     // ends with a sync of the aux stream
            staged = true;
        } else if (pipe_ev) {
            pipe_wait(c);
        }
        k = maxit - 1;
        wait_mon(k);
        const double* mk = hr + offM + 2 * (size_t)k;
        res[k] = std::sqrt(mk[0]) / nb;
        err[k] = gerr[k] >= 0 ? gerr[k] : std::sqrt(mk[1]) / nxt;
    }
    if (k == maxit) k = maxit - 1;
    const int nit = k + 1;                               // niters = k
    if (rs_stream != st) stream_sync(rs_stream);
    if (!x_assigned) throw Error{HGM_E_NOT_ASSIGNED, "Output argument \"x\" not assigned during call (breakdown at k = 1)"};
    if (!staged) stage_out_n<double>(c, x_out, x, n, dev, po);
    if (c->host_stats) {
        const double tot = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        std::fprintf(stderr, "hgm gmres: %d iters, %.1f us total, %.1f us blocked in %ld waits\n", nit, tot * 1e6,
                     (c->wait_s - wait0) * 1e6, c->waits - waits0);
    }
    if (err_out) std::memcpy(err_out, err.data(), sizeof(double) * nit);
    if (res_out) std::memcpy(res_out, res.data(), sizeof(double) * nit);
    if (niters) *niters = nit;
    if (o && o->H_out) std::memcpy(o->H_out, H.data(), sizeof(double) * H.size());
    return HGM_OK;
}

// ============================================================================
// LSQR (lsqr_solver.m) and hybrid LSQR on [A; sqrt(lambda) I] (hybrid_lsqr_solver.m)
// ============================================================================
template <typename T>
int lsqr_t(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* At, const double* b_in,
           const double* xt_in, double tol, int maxit, bool hybrid, double lambda, double* x_out,
           double* err_out, double* res_out, int* niters) {
    check_dims(A, At);
    HGM_REQUIRE(At != nullptr, "At is NULL");
    const PixOrder po = n_order(c, A, At);
    HGM_REQUIRE(b_in != nullptr && xt_in != nullptr, "b and x_true are required");
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    const bool parity = c->num.parity;   // fixed summation orders
    HGM_REQUIRE(!parity || (!dist_n(c) && po.trivial()), "parity mode: single rank, reference pixel order");
    const bool dev = device_ptrs(o, b_in, xt_in, x_out);
    const int64_t m = A->rows, n = A->cols;
    const T* b = stage_in<T>(c, "in_b", b_in, m, dev);
    const T* xt = stage_in_n<T>(c, "in_xt", xt_in, n, dev, po);
    T* x = c->buf<T>("x", n + 1);
    T* w = c->buf<T>("w", n + 1);
    T* v = c->buf<T>("v", n + 1);
    T* u = c->buf<T>("u", m + 1);
    T* un = hybrid ? c->buf<T>("u_n", n + 1) : nullptr;    // lower block of u_aug
    T* t = c->buf<T>("t_m", m + 1);
    T* sl = reinterpret_cast<T*>(c->dscal);
    const T sq = (T)std::sqrt(lambda);
    fill<T>(c, n, x, T(0));
    std::vector<double> err(maxit, 0.0), res(maxit, 0.0);

    sumsq<T>(c, m, b, sl + S_NB);
    nsumsq_diff<T>(c, n, xt, x, sl + S_NXT);
    std::vector<T> hs(4);
    Reader r0(c);
    r0.add(&hs[0], sl + S_NB, sizeof(T));
    r0.add(&hs[1], sl + S_NXT, sizeof(T));
    r0.go();
    const double nb = std::sqrt((double)hs[0]);
    const double nxt = std::sqrt((double)hs[1]);
    // One pass over the operator per iteration: with At = A' value for value on a
    // tiled pixel grid, the step v_hat = A'*u - beta*v (:26) and A*v_hat come out of one pass over
    // At (fused.hip, row epilogue), alpha^2 = ||v_hat||^2 as its side sum, and the next step's
    // A*v_{k+1} (:22) is (A*v_hat) / alpha: an m-vector operation instead of a second pass.
    // wm = [A*v_hat | alpha^2] (m + 1: alpha^2 rides the m-vector all-reduce on a communicator).
    const FusedPlan* fp = agreed_gk_plan<T>(c, A, At, !hybrid && !parity);
    T* wm = fp ? c->buf<T>("gkb_wm", m + 3) : nullptr;        // (+ the partials riding the all-reduce)
    // beta = norm(b) (lsqr_solver.m:7; hybrid: norm([b;0]) = norm(b), hybrid_lsqr_solver.m:9)
    double beta = nb;
    div_scalar<T>(c, m, b, u, (T)beta);                                        // :8  u = b / beta
    if (hybrid) fill<T>(c, n, un, T(0));                                       // u_aug = [b;0]/beta
    if (hybrid) {
        apply_B<T>(c, At, u, v, EPI_ADD, sq, un);                              // A_aug'*u_aug
    } else if (fp) {
        FusedArgs<T> fa = gk_pass_args<T>(u, nullptr, nullptr, wm, m);          // :10 v_hat = A'*u, A*v_hat,
        fa.zraw = v;                                                           //     ||v_hat||^2
        fused_pass<T>(c, At, fp, fa);
        if (dist_n(c)) allreduce(c, wm, m + 1);
    } else {
        apply_B<T>(c, At, u, v, EPI_NONE, T(0), nullptr);                      // :10 v_hat = A'*u
    }
    if (!fp) nsumsq<T>(c, n, v, sl + S_ALPHA);
    double alpha = std::sqrt((double)read1<T>(c, fp ? wm + m : sl + S_ALPHA));   // :11
    div_scalar<T>(c, n, v, v, (T)alpha);                                       // :12
    HGM_HIP(hipMemcpyAsync(w, v, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));   // :14 w = v
    double phi_bar = beta, rho_bar = alpha;                                    // :15-16
    // non-hybrid: the stop test uses phi_bar (host), so the error history (:43) stays on the
    // device and is read once after the loop instead of once per iteration
    T* errh = hybrid ? nullptr : c->buf<T>("lsqr_errh", maxit);
    double *img_ax = nullptr, *img_aw = nullptr;   // (one-pass) A*x, A*w images for :52
    int k = 0;
    // Device-resident scalars (single rank, production kernels): beta and alpha stay on the
    // device as sums of squares, the SpMV epilogues read them there (PendNorm::asq), and the
    // Givens rotation (:31-38) and the stop test (:44-46) run in a one-thread kernel, in the same
    // double arithmetic as the host loop below -- the same bits, with no host round trip per
    // iteration.  The host reads the stop flag once per batch of iterations (none when tol <= 0
    // cannot stop early); an iteration enqueued past the stop leaves x and w untouched.
    const bool dev_scalars = !fp && !hybrid && !parity && !dist_n(c) && c->num.lsqr_dev;
    double c_x = 0, c_w = 0;                       // phi/rho, theta/rho of :40-41 (lsqr_rotate)
    if (fp || dev_scalars) {
        // (one pass per iteration: device-resident scalars as above, on a communicator too -- alpha^2
        // rides the m-vector all-reduce, beta^2 is a sum over the replicated m-vector)
        double* st = c->buf<double>("lsqr_st", 4);
        double* phib = c->buf<double>("lsqr_phib", maxit);
        T* coef = c->buf<T>("lsqr_coef", 2);
        const double st0[4] = {rho_bar, phi_bar, 0.0, 0.0};
        h2d(c, st, st0, sizeof(st0));
        // HGM_OPT_LSQR_DEV = 0: the same pass with host scalars -- beta^2 and alpha^2 read back per
        // iteration, the rotation and the stop test on the host in the same double arithmetic as
        // k_lsqr_rot (the coefficients uploaded for lsqr_step), so the iterates keep their bits
        const bool host_sc = fp && !c->num.lsqr_dev;
        const int batch = tol > 0 && !host_sc ? 8 : maxit;
        const double* stop_slot = host_sc ? nullptr : st + 2;
        int stop = 0;
        if (fp) {
            const FusedArgs<T> fa = gk_pass_args<T>(u, v, sl + S_BETA, wm, m);   // v_k in, v_hat_{k+1} in place
            // On a communicator the error partial ||x - x_true||^2 (:43) rides the next iteration's
            // m-vector all-reduce: one collective per iteration instead of two (the stop test uses
            // phi_bar, replicated)
            Ridden<T> rd = ride_begin<T>(c, dist_n(c) && !host_sc, wm, m, errh, nullptr);
            // the final residual (:52) from A*x kept alongside x (A*v_k is the pass's A*v_hat / alpha):
            // no SpMV after the loop (HGM_OPT_LSQR_RES_IMG)
            if (c->num.lsqr_res_img) {
                img_ax = c->buf<double>("lsqr_ax", m + 1);
                img_aw = c->buf<double>("lsqr_aw", m + 1);
                lsqr_img<T>(c, m, wm, wm + m, coef, st, 0, img_ax, img_aw, true);
            }
            stop = batched_iterations(c, maxit, batch, stop_slot, [&](int k) {
                int host_stop = 0;
                gkb_mstep_div<T>(c, m, wm, wm + m, u, t, nullptr, sl + S_BETA, false);   // :22-24
                fused_pass<T>(c, At, fp, fa);                                        // :26-27 (+ A*v_hat)
                if (dist_n(c)) allreduce(c, wm, rd.count(m, k));
                if (host_sc) {
                    T ss[2] = {T(0), T(0)};
                    Reader rr(c);
                    rr.add(&ss[0], sl + S_BETA, sizeof(T));
                    rr.add(&ss[1], wm + m, sizeof(T));
                    rr.go();
                    beta = std::sqrt((double)ss[0]);                                 // :23
                    alpha = std::sqrt((double)ss[1]);                                // :27
                    lsqr_rotate(beta, alpha, rho_bar, phi_bar, c_x, c_w);            // :31-38
                    const T cf[2] = {(T)c_x, (T)c_w};
                    h2d_pinned(c, coef, cf, sizeof(cf));    // the next Reader syncs past its use
                    res[k] = std::fabs(phi_bar) / nb;                                // :44
                    if (res[k] <= tol) host_stop = k + 1;                            // :46 (<=)
                } else {
                    lsqr_rot<T>(c, sl + S_BETA, wm + m, st, coef, phib, k, nb, tol,  // :31-38, :44-46
                                k > 0 ? rd.into(k - 1) : ScalarCopy<T>{});
                }
                lsqr_step<T>(c, n, x, w, v, wm + m, coef, st, k, xt, rd.e ? rd.e : errh + k);   // :28, :40-41, :43
                rd.last = k;
                if (img_ax) lsqr_img<T>(c, m, wm, wm + m, coef, st, k, img_ax, img_aw, false);
                if (dist_n(c) && !rd.e) allreduce(c, errh + k, 1);
                return host_stop;
            });
            ride_end(c, rd);
        } else {
            PendNorm<T> pa, pb;
            pa.asq = sl + S_ALPHA;                     // A*v - alpha*u
            pb.asq = sl + S_BETA;                      // A'*u - beta*v
            stop = batched_iterations(c, maxit, batch, stop_slot, [&](int k) {
                spmv<T>(c, A, v, t, EPI_SUB, T(0), u, KC_SPMV_A, nullptr, &pa);     // :22
                sumsq<T>(c, m, t, sl + S_BETA);                                      // :23
                div_sqrt<T>(c, m, t, u, sl + S_BETA);                                // :24
                spmv<T>(c, At, u, v, EPI_SUB, T(0), v, KC_SPMV_B, nullptr, &pb);     // :26
                sumsq<T>(c, n, v, sl + S_ALPHA);                                     // :27
                lsqr_rot<T>(c, sl + S_BETA, sl + S_ALPHA, st, coef, phib, k, nb, tol);   // :31-38, :44-46
                lsqr_step<T>(c, n, x, w, v, sl + S_ALPHA, coef, st, k, xt, errh + k);     // :28, :40-41, :43
                return 0;
            });
        }
        k = stop > 0 ? stop - 1 : maxit;
        if (!host_sc) read_phib(c, phib, maxit, k, nb, res);                         // :44
    }
    for (; !dev_scalars && !fp && k < maxit; ++k) {
        // :22-24  u_hat = A*v - alpha*u ; beta = norm(u_hat) ; u = u_hat / beta
        apply_A<T>(c, A, v, t, EPI_SUB, (T)alpha, u);
        sumsq<T>(c, m, t, sl + S_BETA);
        if (hybrid) {
            // lower block of u_hat: (sqrt(lambda)*v) - (alpha*u_n), same norm as the upper block
            T* tl = c->buf<T>("t_n", n + 1);
            fill<T>(c, n, tl, T(0));
            epilogue<T>(c, n, tl, EPI_ADD, sq, v);                     // tl = 0 + sq*v (exact: sq*v)
            epilogue<T>(c, n, tl, EPI_SUB, (T)alpha, un);              // tl = tl - alpha*u_n
            if (parity) {
                // norm of the augmented [u_m; u_n] (:23) in one fixed order over the concatenation
                fixed_reduce<T>(c, 1, m, t, t, n, tl, tl, sl + S_BETA);
                HGM_HIP(hipMemsetAsync(sl + S_AUX, 0, sizeof(T), c->stream));
            } else {
                nsumsq<T>(c, n, tl, sl + S_AUX);
            }
            Reader rr(c);
            rr.add(&hs[0], sl + S_BETA, sizeof(T));
            rr.add(&hs[1], sl + S_AUX, sizeof(T));
            rr.go();
            beta = std::sqrt((double)(hs[0] + hs[1]));
            div_scalar<T>(c, m, t, u, (T)beta);
            div_scalar<T>(c, n, tl, un, (T)beta);
            // :26 v_hat = A_aug'*u_aug - beta*v = (A'*u + sq*un) - beta*v
            T* vh = c->buf<T>("t_n2", n + 1);   // A_aug'*u_aug reads v in the epilogue: not in place
            apply_B<T>(c, At, u, vh, EPI_ADD, sq, un);
            epilogue<T>(c, n, vh, EPI_SUB, (T)beta, v);
            HGM_HIP(hipMemcpyAsync(v, vh, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));
        } else {
            beta = std::sqrt((double)read1<T>(c, sl + S_BETA));
            div_scalar<T>(c, m, t, u, (T)beta);
            // :26 v_hat = A'*u - beta*v   (in place is safe: row i reads v(i) only in its epilogue)
            apply_B<T>(c, At, u, v, EPI_SUB, (T)beta, v);
        }
        nsumsq<T>(c, n, v, sl + S_ALPHA);
        alpha = std::sqrt((double)read1<T>(c, sl + S_ALPHA));                 // :27
        div_scalar<T>(c, n, v, v, (T)alpha);                                   // :28
        lsqr_rotate(beta, alpha, rho_bar, phi_bar, c_x, c_w);                  // :31-38 (host scalars)
        lsqr_update<T>(c, n, x, w, v, (T)c_x, (T)c_w);                         // :40-41
        nsumsq_diff<T>(c, n, x, xt, hybrid ? sl + S_ERR : errh + k);
        if (hybrid) {
            apply_A<T>(c, A, x, t, EPI_RSUB, T(0), b);                        // hybrid :43  b - A*x
            sumsq<T>(c, m, t, sl + S_RES);
            Reader rr(c);
            rr.add(&hs[0], sl + S_ERR, sizeof(T));
            rr.add(&hs[1], sl + S_RES, sizeof(T));
            rr.go();
            err[k] = std::sqrt((double)hs[0]) / nxt;
            res[k] = std::sqrt((double)hs[1]) / nb;
            if (res[k] < tol) break;                                           // hybrid :45 (<)
        } else {
            res[k] = std::fabs(phi_bar) / nb;                                  // :44 (:43 below)
            if (res[k] <= tol) break;                                          // :46 (<=)
        }
    }
    if (k == maxit) k = maxit - 1;
    const int nit = k + 1;
    if (!hybrid) {
        std::vector<T> eh(nit);
        Reader re(c);
        re.add(eh.data(), errh, sizeof(T) * nit);
        re.go();
        for (int i = 0; i < nit; ++i) err[i] = std::sqrt((double)eh[i]) / nxt;   // :43
        if (img_ax) {
            // :52 norm(b - A*x) from the kept image (replicated m-vector: no collective)
            double* b64 = c->buf<double>("lsqr_b64", m + 1);
            if constexpr (std::is_same_v<T, double>) {
                HGM_HIP(hipMemcpyAsync(b64, b, sizeof(double) * m, hipMemcpyDeviceToDevice, c->stream));
            } else {
                convert_back<T>(c, m, b, b64);
            }
            double* rs = c->buf<double>("lsqr_rs", 1);
            sumsq_diff<double>(c, m, b64, img_ax, rs);
            double hv = 0;
            Reader rr(c);
            rr.add(&hv, rs, sizeof(double));
            rr.go();
            res[nit - 1] = std::sqrt(hv) / nb;
        } else {
            apply_A<T>(c, A, x, t, EPI_RSUB, T(0), b);                        // :52 exact final residual
            sumsq<T>(c, m, t, sl + S_RES);
            res[nit - 1] = std::sqrt((double)read1<T>(c, sl + S_RES)) / nb;
        }
    }
    stage_out_n<T>(c, x_out, x, n, dev, po);
    if (err_out) std::memcpy(err_out, err.data(), sizeof(double) * nit);
    if (res_out) std::memcpy(res_out, res.data(), sizeof(double) * nit);
    if (niters) *niters = nit;
    return HGM_OK;
}

// ============================================================================
// LSMR (lsmr_solver.m)
// ============================================================================
template <typename T>
int lsmr_t(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* At, const double* b_in,
           const double* xt_in, double tol, int maxit, double* x_out, double* err_out, double* res_out,
           double* ar_out, int* iters) {
    check_dims(A, At);
    HGM_REQUIRE(At != nullptr, "At is NULL");
    const PixOrder po = n_order(c, A, At);
    HGM_REQUIRE(b_in != nullptr, "b is required");
    const bool parity = c->num.parity;   // fixed summation orders
    HGM_REQUIRE(!parity || (!dist_n(c) && po.trivial()), "parity mode: single rank, reference pixel order");
    const bool dev = device_ptrs(o, b_in, xt_in, x_out);
    const int64_t m = A->rows, n = A->cols;
    if (maxit <= 0) maxit = (int)std::min<int64_t>(m, n);                    // :5 default min(m,n)
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    const T* b = stage_in<T>(c, "in_b", b_in, m, dev);
    const T* xt = stage_in_n<T>(c, "in_xt", xt_in, n, dev, po);
    T* x = c->buf<T>("x", n + 1);
    T* v = c->buf<T>("v", n + 1);
    T* h = c->buf<T>("h", n + 1);
    T* hbar = c->buf<T>("hbar", n + 1);
    T* u = c->buf<T>("u", m + 1);
    T* r = c->buf<T>("t_m", m + 1);
    T* atr = c->buf<T>("t_n", n + 1);
    T* sl = reinterpret_cast<T*>(c->dscal);
    fill<T>(c, n, x, T(0));                                                    // :7
    fill<T>(c, n, hbar, T(0));                                                 // :26
    std::vector<double> err(maxit, std::numeric_limits<double>::quiet_NaN());  // :28
    std::vector<double> res(maxit, 0.0), ar(maxit, 0.0);
    std::vector<T> hs(4);

    sumsq<T>(c, m, b, sl + S_NB);
    if (xt) nsumsq_diff<T>(c, n, xt, x, sl + S_NXT);
    // ||A||_F (lsmr_solver.m:71, loop-invariant): cached per matrix (parity mode: recomputed in
    // the fixed order, not cached)
    double normA = A->fro;
    if (A->fro < 0 || parity) {
        double* f = reinterpret_cast<double*>(c->dscal) + 64;
        if (A->dtype == HGM_F32) fro2<float>(c, A, f); else fro2<double>(c, A, f);
        if (dist_n(c)) allreduce(c, f, 1);
        double fv;
        Reader rf(c);
        rf.add(&fv, f, sizeof(double));
        rf.go();
        normA = std::sqrt(fv);
        if (!parity) const_cast<hgm_mat*>(A)->fro = normA;
    }
    Reader r0(c);
    r0.add(&hs[0], sl + S_NB, sizeof(T));
    if (xt) r0.add(&hs[1], sl + S_NXT, sizeof(T));
    r0.go();
    const double nb = std::sqrt((double)hs[0]);
    const double nxt = xt ? std::sqrt((double)hs[1]) : 0.0;
    // Monitors from kept products (default; HGM_EXPLICIT_RESIDUAL applies the two extra SpMVs
    // of :69 and :71 instead): the raw products A*v_k and A'*u_{k+1} of the bidiagonalisation
    // are kept, and the images A*x, A'A*x follow the x/h/hbar recurrences (lsmr_monitor).  The
    // iterates u, v, x, h, hbar are the same bits either way (the epilogues below are the
    // fused ones, applied as a separate pass).
    const bool kept = !(o && (o->flags & HGM_EXPLICIT_RESIDUAL)) && !parity;
    T *Av = nullptr, *Atu0 = nullptr, *Atu1 = nullptr, *Atb = nullptr;
    double *Ihm = nullptr, *Ihbm = nullptr, *Ixm = nullptr, *Ihn = nullptr, *Ihbn = nullptr, *Ixn = nullptr;
    double* dmon = reinterpret_cast<double*>(c->dscal) + 72;   // [||r||^2, ||A'r||^2]
    if (kept) {
        Av = c->buf<T>("lsmr_Av", m + 1);
        Atu0 = c->buf<T>("lsmr_Atu0", n + 1);
        Atu1 = c->buf<T>("lsmr_Atu1", n + 1);
        Atb = c->buf<T>("lsmr_Atb", n + 1);
        Ihm = c->buf<double>("lsmr_Ihm", m + 1);
        Ihbm = c->buf<double>("lsmr_Ihbm", m + 1);
        Ixm = c->buf<double>("lsmr_Ixm", m + 1);
        Ihn = c->buf<double>("lsmr_Ihn", n + 1);
        Ihbn = c->buf<double>("lsmr_Ihbn", n + 1);
        Ixn = c->buf<double>("lsmr_Ixn", n + 1);
        fill<double>(c, m, Ixm, 0.0);                                          // A*x_0 = 0
        fill<double>(c, n, Ixn, 0.0);                                          // A'A*x_0 = 0
    }
    // One pass over the operator per iteration (as lsqr_t): the step :38-39 and
    // A*v_hat in one pass over At, A*v_{k+1} (:34, the kept A*v) = (A*v_hat) / alpha.
    const FusedPlan* fp = agreed_gk_plan<T>(c, A, At, !parity);
    T* wm = fp ? c->buf<T>("gkb_wm", m + 3) : nullptr;                         // [A*v_hat | alpha^2 | ridden]
    HGM_HIP(hipMemcpyAsync(u, b, sizeof(T) * m, hipMemcpyDeviceToDevice, c->stream));   // :10
    double beta = nb;                                                          // :11
    if (beta > 0) div_scalar<T>(c, m, u, u, (T)beta);                          // :12
    T* v0 = kept ? Atu0 : v;                                                   // raw A'*u_0 kept
    if (fp) {
        FusedArgs<T> fa = gk_pass_args<T>(u, nullptr, nullptr, wm, m);          // :14 (+ A*v_hat, ||v_hat||^2)
        fa.zraw = v0;
        fused_pass<T>(c, At, fp, fa);
        if (dist_n(c)) allreduce(c, wm, m + 1);
    } else {
        apply_B<T>(c, At, u, v0, EPI_NONE, T(0), nullptr);                     // :14
        nsumsq<T>(c, n, v0, sl + S_ALPHA);
    }
    double alpha = std::sqrt((double)read1<T>(c, fp ? wm + m : sl + S_ALPHA));   // :15
    // A'*b for the monitors' A'r = A'b - A'A*x: beta * A'*u_0 (u_0 = b / beta, :12-14), the product
    // just formed, instead of one more pass over the operator per solve (equal up to rounding)
    if (kept) scale<T>(c, n, Atu0, Atb, (T)beta);
    if (alpha > 0) div_scalar<T>(c, n, v0, v, (T)alpha);                       // :16
    else if (kept) HGM_HIP(hipMemcpyAsync(v, v0, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));
    // The rotations' state (lsmr_rotate, internal.h): [alpha, alphabar, rho, rhobar, cbar, sbar, zetabar
    // = alpha*beta (:19-23), theta/rho of the previous :67, the device loop's stop slot]
    double rot[9] = {alpha, alpha, 1, 1, 1, 0, alpha * beta, 0.0, 0.0};
    HGM_HIP(hipMemcpyAsync(h, v, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));   // :25
    // tol <= 0: `res < tol` (:76) can never hold, so the monitors stay on the device and are
    // read once after the loop instead of once per iteration
    // (and with the device-resident scalars below at any tol)
    const bool defer_mon = kept && (!(tol > 0) || (fp && c->num.lsqr_dev));
    double* dmonh = defer_mon ? c->buf<double>("lsmr_monh", 2 * (size_t)maxit) : nullptr;
    T* errh = defer_mon ? c->buf<T>("lsmr_errh", maxit) : nullptr;
    auto monitors = [&](int kk, double m0, double m1, double e2) {
        const double nr = std::sqrt(m0);
        res[kk] = nr / (nb + EPSD);                                            // :70
        ar[kk] = std::sqrt(m1) / (normA * std::max(nr, EPSD));                 // :71
        if (xt) err[kk] = std::sqrt(e2) / nxt;                                 // :72-73
    };
    int k = 0;
    // Device-resident scalars (the one-pass path with kept monitors): beta and alpha
    // stay on the device as sums of squares, the rotations :42-67 run in one thread (lsmr_rot, the
    // loop's double arithmetic below), the n-space step divides v by alpha and carries the error sum,
    // and the stop test :76 runs on the device after the monitors -- no host round trip per
    // iteration.  The host reads the stop flag once per batch of 8 iterations (none with tol <= 0);
    // an iteration enqueued past the stop leaves x untouched, and its histories are dropped.
    const bool dev_scalars = fp && kept && c->num.lsqr_dev;
    if (dev_scalars) {
        // fp32 solves: the n-space monitor carries A'r in T (lsmr_monitor_r; Ir_0 = A'b)
        constexpr bool img_t = std::is_same_v<T, float>;
        T *Ihn_t = nullptr, *Ihbn_t = nullptr, *Irn_t = nullptr;
        if constexpr (img_t) {
            Ihn_t = c->buf<T>("lsmr_Ihn_t", n + 4);
            Ihbn_t = c->buf<T>("lsmr_Ihbn_t", n + 4);
            Irn_t = c->buf<T>("lsmr_Irn_t", n + 4);
            HGM_HIP(hipMemcpyAsync(Irn_t, Atb, sizeof(T) * n, hipMemcpyDeviceToDevice, c->stream));
        }
        double* st = c->buf<double>("lsmr_st", 9);
        double* cfm = c->buf<double>("lsmr_cf", 10);
        double* cfn = cfm + 5;
        T* coef = c->buf<T>("lsmr_coef", 3);
        h2d(c, st, rot, sizeof(rot));
        FusedArgs<T> fa = gk_pass_args<T>(u, v, sl + S_BETA, wm, m);
        // On a communicator the n-space partials of iteration k -- ||x - x_true||^2 (:72) and, in
        // fp64, ||A'r||^2 (:71) -- ride iteration k+1's m-vector all-reduce: one collective per
        // iteration instead of three (fp32: two).  The stop test (:76) reads only the replicated
        // m-space residual.
        Ridden<T> rd = ride_begin<T>(c, dist_n(c), wm, m, xt ? errh : nullptr, dmonh);
        const int stop = batched_iterations(c, maxit, tol > 0 ? 8 : maxit, tol > 0 ? st + 8 : nullptr, [&](int k) {
            gkb_mstep_div<T>(c, m, wm, wm + m, u, r, Av, sl + S_BETA, true);  // :34-36 (+ kept A*v_k)
            fa.zraw = Atu1;                                                   // A'*u_{k+1} (kept)
            fused_pass<T>(c, At, fp, fa);                                     // :38-39 (+ A*v_hat)
            if (dist_n(c)) allreduce(c, wm, rd.count(m, k));
            lsmr_rot<T>(c, sl + S_BETA, wm + m, st, coef, cfm, cfn,           // :42-67 scalars
                        k > 0 ? rd.into(k - 1) : ScalarCopy<T>{});
            double* dm = dmonh + 2 * (size_t)k;
            T* e_out = xt ? (rd.e ? rd.e : errh + k) : nullptr;
            double* d_out = rd.d ? rd.d : dm + 1;
            // (fp32: the n-space step and the n-space monitor in one launch when it applies)
            const bool nmon = img_t && lsmr_step_mon<T>(c, n, x, h, hbar, v, wm + m, coef, st, k, xt, e_out,
                                                        Atu1, Atu0, Ihn_t, Ihbn_t, Irn_t, k == 0, d_out, cfn);
            if (!nmon) lsmr_step<T>(c, n, x, h, hbar, v, wm + m, coef, st, k, xt, e_out);   // :40, :61-67, :72
            rd.last = k;
            if (xt && dist_n(c) && !rd.e) allreduce(c, errh + k, 1);
            lsmr_monitor<T>(c, m, Av, nullptr, 0, 0, Ihm, Ihbm, Ixm, b, 0, 0, 0, k == 0, dm, cfm);
            if (!nmon && img_t) lsmr_monitor_r<T>(c, n, Atu1, Atu0, Ihn_t, Ihbn_t, Irn_t, k == 0, d_out, cfn);
            else if (!nmon) lsmr_monitor<T>(c, n, Atu1, Atu0, 0, 0, Ihn, Ihbn, Ixn, Atb, 0, 0, 0, k == 0, d_out, cfn);
            if (dist_n(c) && !rd.d) allreduce(c, dm + 1, 1);
            std::swap(Atu0, Atu1);
            if (tol > 0) lsmr_stop(c, dm, nb, tol, st, k);                   // :76
            return 0;
        });
        ride_end(c, rd);
        k = stop > 0 ? stop - 1 : maxit;
    }
    for (k = dev_scalars ? k : 0; !dev_scalars && k < maxit; ++k) {
        if (fp) {
            // :34 A*v_k = (A*v_hat)/alpha_k (kept), u = A*v - alpha*u, ||u||^2
            gkb_mstep<T>(c, m, wm, wm + m, u, r, kept ? Av : nullptr, sl + S_BETA);
            beta = std::sqrt((double)read1<T>(c, sl + S_BETA));               // :35
            if (beta > 0) div_scalar<T>(c, m, r, u, (T)beta);                  // :36
            else HGM_HIP(hipMemcpyAsync(u, r, sizeof(T) * m, hipMemcpyDeviceToDevice, c->stream));
            FusedArgs<T> fa = gk_pass_args<T>(u, v, sl + S_BETA, wm, m);       // :38 v = A.'*u - beta*v, one pass
            fa.zraw = kept ? Atu1 : nullptr;                                   // A'*u_{k+1} (kept)
            fused_pass<T>(c, At, fp, fa);                                      // (+ ||v||^2, :39)
            if (dist_n(c)) allreduce(c, wm, m + 1);
            alpha = std::sqrt((double)read1<T>(c, wm + m));                    // :39
        } else {
            if (kept) {
                apply_A<T>(c, A, v, Av, EPI_NONE, T(0), nullptr);              // A*v_k (kept)
                epilogue_to<T>(c, m, Av, u, EPI_SUB, (T)alpha, u);             // :34 u = A*v - alpha*u
            } else {
                apply_A<T>(c, A, v, u, EPI_SUB, (T)alpha, u);                  // :34 u = A*v - alpha*u
            }
            sumsq<T>(c, m, u, sl + S_BETA);
            beta = std::sqrt((double)read1<T>(c, sl + S_BETA));               // :35
            if (beta > 0) div_scalar<T>(c, m, u, u, (T)beta);                  // :36
            if (kept) {
                apply_B<T>(c, At, u, Atu1, EPI_NONE, T(0), nullptr);           // A'*u_{k+1} (kept)
                epilogue_to<T>(c, n, Atu1, v, EPI_SUB, (T)beta, v);            // :38 v = A.'*u - beta*v
            } else {
                apply_B<T>(c, At, u, v, EPI_SUB, (T)beta, v);                  // :38 v = A.'*u - beta*v
            }
            nsumsq<T>(c, n, v, sl + S_ALPHA);
            alpha = std::sqrt((double)read1<T>(c, sl + S_ALPHA));             // :39
        }
        if (alpha > 0) div_scalar<T>(c, n, v, v, (T)alpha);                    // :40
        double cf[3], cfm[5], cfn[5];                  // [c_hbar, c_x, c_h]; the monitors' [c1, c0, f, e, cx]
        lsmr_rotate(beta, alpha, rot, cf, cfm, cfn);                           // :42-67 scalars
        lsmr_update<T>(c, n, x, h, hbar, v, (T)cf[0], (T)cf[1], (T)cf[2], k == 0);   // :61-67
        double mon[2] = {0.0, 0.0};
        Reader rr(c);
        if (kept) {
            // :69 ||b - A*x||^2 and :71 ||A'b - A'A*x||^2 from the kept images
            double* dm = defer_mon ? dmonh + 2 * (size_t)k : dmon;
            lsmr_monitor<T>(c, m, Av, nullptr, cfm[0], cfm[1], Ihm, Ihbm, Ixm, b, cfm[2], cfm[3], cfm[4], k == 0, dm);
            lsmr_monitor<T>(c, n, Atu1, Atu0, cfn[0], cfn[1], Ihn, Ihbn, Ixn, Atb, cfn[2], cfn[3], cfn[4], k == 0,
                            dm + 1);
            if (dist_n(c)) allreduce(c, dm + 1, 1);
            std::swap(Atu0, Atu1);
            if (!defer_mon) rr.add(mon, dmon, sizeof(double) * 2);
        } else {
            apply_A<T>(c, A, x, r, EPI_RSUB, T(0), b);                         // :69 r = b - A*x
            sumsq<T>(c, m, r, sl + S_RES);
            apply_B<T>(c, At, r, atr, EPI_NONE, T(0), nullptr);                // :71 A.'*r
            nsumsq<T>(c, n, atr, sl + S_AR);
            rr.add(&hs[0], sl + S_RES, sizeof(T));
            rr.add(&hs[1], sl + S_AR, sizeof(T));
        }
        if (xt) nsumsq_diff<T>(c, n, x, xt, defer_mon ? errh + k : sl + S_ERR);
        if (defer_mon) continue;
        if (xt) rr.add(&hs[2], sl + S_ERR, sizeof(T));
        rr.go();
        if (!kept) {
            mon[0] = (double)hs[0];
            mon[1] = (double)hs[1];
        }
        monitors(k, mon[0], mon[1], xt ? (double)hs[2] : 0.0);
        if (res[k] < tol) break;                                               // :76 (<)
    }
    if (k == maxit) k = maxit - 1;
    const int nit = k + 1;
    if (defer_mon) {
        std::vector<double> mh(2 * (size_t)nit);
        std::vector<T> eh(nit, T(0));
        Reader re(c);
        re.add(mh.data(), dmonh, sizeof(double) * mh.size());
        if (xt) re.add(eh.data(), errh, sizeof(T) * nit);
        re.go();
        for (int i = 0; i < nit; ++i) monitors(i, mh[2 * i], mh[2 * i + 1], (double)eh[i]);
    }
    stage_out_n<T>(c, x_out, x, n, dev, po);
    if (err_out) std::memcpy(err_out, err.data(), sizeof(double) * nit);
    if (res_out) std::memcpy(res_out, res.data(), sizeof(double) * nit);
    if (ar_out) std::memcpy(ar_out, ar.data(), sizeof(double) * nit);
    if (iters) *iters = nit;
    return HGM_OK;
}

// ============================================================================
// hybrid LSMR (hybrid_lsmr_solver.m)
// ============================================================================
int hybrid_lsmr(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* At, const double* b_in,
                const double* xt_in, double tol, int maxit, double lambda, double* x_out, double* err_out,
                double* res_out, int* niters) {
    check_dims(A, At);
    HGM_REQUIRE(At != nullptr, "At is NULL");
    const PixOrder po = n_order(c, A, At);
    HGM_REQUIRE(A->dtype == HGM_F64, "hybrid LSMR is fp64");
    HGM_REQUIRE(!c->num.parity || (!dist_n(c) && po.trivial()), "parity mode: single rank, reference pixel order");
    HGM_REQUIRE(b_in != nullptr && xt_in != nullptr, "b and x_true are required");
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    const bool dev = device_ptrs(o, b_in, xt_in, x_out);
    const int64_t m = A->rows, n = A->cols;
    const int64_t ldv = round_up(n > 0 ? n : 1, 64);
    const double* b = stage_in<double>(c, "in_b", b_in, m, dev);
    const double* xt = stage_in_n<double>(c, "in_xt", xt_in, n, dev, po);
    double* V = c->buf<double>("Q", (size_t)ldv * maxit);
    double* x = c->buf<double>("x", n + 1);
    double* u = c->buf<double>("u", m + 1);
    double* t = c->buf<double>("t_m", m + 1);
    double* yd = c->buf<double>("y", maxit + 8);
    double* sl = c->dscal;
    fill<double>(c, n, x, 0.0);
    std::vector<double> err(maxit, 0.0), res(maxit, 0.0);
    std::vector<double> Bk((size_t)(maxit + 1) * maxit, 0.0);                  // :11
    auto BK = [&](int i, int j) -> double& { return Bk[(size_t)j * (maxit + 1) + i]; };

    sumsq<double>(c, m, b, sl + S_NB);
    nsumsq_diff<double>(c, n, xt, x, sl + S_NXT);
    read_scalars(c, 0, 2);
    const double nb = std::sqrt(c->hscal[S_NB]);
    const double nxt = std::sqrt(c->hscal[S_NXT]);
    const double beta1 = nb;                                                   // :7
    div_scalar<double>(c, m, b, u, beta1);                                          // :8
    double* v0 = V;
    apply_B<double>(c, At, u, v0, EPI_NONE, 0.0, nullptr);                          // :13
    nsumsq<double>(c, n, v0, sl + S_ALPHA);
    double alpha1 = std::sqrt(read1<double>(c, sl + S_ALPHA));                      // :14
    div_scalar<double>(c, n, v0, v0, alpha1);                                       // :15-16
    int k = 0;
    std::vector<double> y;
    for (k = 0; k < maxit; ++k) {
        double* vk = V + (int64_t)k * ldv;
        BK(k, k) = alpha1;                                                     // :23
        apply_A<double>(c, A, vk, t, EPI_SUB, alpha1, u);                           // :24
        sumsq<double>(c, m, t, sl + S_BETA);
        const double beta_k = std::sqrt(read1<double>(c, sl + S_BETA));            // :25
        div_scalar<double>(c, m, t, u, beta_k);                                     // :26
        BK(k + 1, k) = beta_k;                                                 // :27
        if (k < maxit - 1) {                                                   // :29
            double* vn = V + (int64_t)(k + 1) * ldv;
            apply_B<double>(c, At, u, vn, EPI_SUB, beta_k, vk);                     // :30
            nsumsq<double>(c, n, vn, sl + S_ALPHA);
            const double a1 = std::sqrt(read1<double>(c, sl + S_ALPHA));            // :31
            div_scalar<double>(c, n, vn, vn, a1);                                   // :32-33
            alpha1 = a1;                                                       // :34
        }
        const int kk = k + 1;
        // :37-44  LHS = (Bk'*Bk)^2 + (alpha_k1*beta_k1)^2 e1 e1' + lambda I ; RHS = B_k(1,1) beta1 (Bk'*Bk) e1
        y.assign(kk, 0.0);
        dense::proj_hybrid_lsmr(Bk.data(), maxit + 1, kk, alpha1, beta_k, beta1, lambda, y.data());   // :44
        h2d_pinned(c, yd, y.data(), sizeof(double) * kk);
        gemv<double>(c, n, kk, V, ldv, yd, x, 0);                                   // :45
        nsumsq_diff<double>(c, n, x, xt, sl + S_ERR);                               // :47
        apply_A<double>(c, A, x, t, EPI_RSUB, 0.0, b);                              // :48
        sumsq<double>(c, m, t, sl + S_RES);
        read_scalars(c, S_RES, 2);
        res[k] = std::sqrt(c->hscal[S_RES]) / nb;
        err[k] = std::sqrt(c->hscal[S_ERR]) / nxt;
        if (res[k] <= tol) break;                                              // :50
    }
    if (k == maxit) k = maxit - 1;
    const int nit = k + 1;
    stage_out_n<double>(c, x_out, x, n, dev, po);
    if (err_out) std::memcpy(err_out, err.data(), sizeof(double) * nit);
    if (res_out) std::memcpy(res_out, res.data(), sizeof(double) * nit);
    if (niters) *niters = nit;
    return HGM_OK;
}

// ============================================================================
// Arnoldi for GCV (gcv_function.m:3-33)
// ============================================================================
int arnoldi(hgm_ctx* c, const hgm_mat* A, const hgm_mat* B, const double* b_in, int kg, int side,
            double btol, int orth, double* H_out, double* beta_out, int* kdone) {
    check_dims(A, B);
    HGM_REQUIRE(B != nullptr, "B is NULL");
    (void)n_order(c, A, B);   // H does not depend on the stored pixel order (up to rounding)
    HGM_REQUIRE(A->dtype == HGM_F64, "Arnoldi is fp64");
    HGM_REQUIRE(kg >= 1, "k must be >= 1");
    const int64_t m = A->rows, n = A->cols;
    const bool nspace = side == HGM_SIDE_BA;
    const int64_t dim = nspace ? n : m;
    const bool dist = nspace && dist_n(c);
    HGM_REQUIRE(!c->num.parity || !dist_n(c), "parity mode: single rank");
    const double* b = stage_in<double>(c, "in_b", b_in, m, false);
    const KrylovBasis kb = krylov_basis(c, "Q", dim, kg + 1, dist);
    double* Q = kb.Q;
    const int64_t ldq = kb.ld;
    double* Hd = c->buf<double>("H", (size_t)(kg + 1) * kg);
    double* t = c->buf<double>("t_m", m + 1);
    double* tn = c->buf<double>("t_n", n + 1);
    HGM_HIP(hipMemsetAsync(Hd, 0, sizeof(double) * (kg + 1) * kg, c->stream));
    start_residual(c, B, b, nspace, kb, dslot<double>(c, S_BETA));                 // :5 / :8  r0
    const double beta = std::sqrt(read1<double>(c, dslot<double>(c, S_BETA)));           // :12
    div_scalar<double>(c, dim, Q, Q, beta);                                         // :15
    std::vector<double> H((size_t)(kg + 1) * kg, 0.0);
    int done = 0;
    const FusedPlan* fplan = nspace ? nullptr : fused_ab_plan(c, A, B);        // A*(B*q) in one pass
    // The steps are enqueued back to back, with no host round trip per step: the breakdown
    // test H(k+1,k) < btol runs on the host afterwards, and the steps past a breakdown (which
    // wrote only Q(:,>k+1) and H(:,>k) on the device) are discarded.
    for (int k = 0; k < kg; ++k) {
        double* qk = Q + (int64_t)k * ldq;
        double* v = Q + (int64_t)(k + 1) * ldq;
        apply_M(c, A, B, fplan, nspace, qk, nspace ? t : tn, v);      // :22 B*(A*Q(:,k)) / :20 A*(B*Q(:,k))
        double* Hcol = Hd + (int64_t)k * (kg + 1);
        if (orth == HGM_CGS2) cgs2<double>(c, dim, Q, ldq, k, Hcol, dist);
        else mgs<double>(c, dim, Q, ldq, k, Hcol, dist);                            // :25-31
    }
    std::vector<double> Hall((size_t)(kg + 1) * kg);
    Reader rd(c);
    rd.add(Hall.data(), Hd, sizeof(double) * Hall.size());
    rd.go();
    for (int k = 0; k < kg; ++k) {
        std::memcpy(&H[(size_t)k * (kg + 1)], &Hall[(size_t)k * (kg + 1)], sizeof(double) * (k + 2));
        done = k + 1;
        if (H[(size_t)k * (kg + 1) + k + 1] < btol) {                          // :30  H(k+1,k) < 1e-12 -> break
            // the reference breaks before Q(:,k+1) = v/H(k+1,k); H(k+1,k) keeps its value
            break;
        }
    }
    if (H_out) std::memcpy(H_out, H.data(), sizeof(double) * H.size());
    if (beta_out) *beta_out = beta;
    if (kdone) *kdone = done;
    return HGM_OK;
}

// ============================================================================
// Lambda sweep of the hybrid PTR solvers: one Arnoldi for every lambda
// ============================================================================
// In ABgmres_hybrid_bounds.m:24-41 / BAgmres_hybrid_bounds.m:24-40 lambda enters only the k x k
// projected solve yk = (Hk'*Hk + lambda*eye(k)) \ (Hk'*tk): Q, H and the kept products V = B*Q (AB)
// or Q (BA) and W = A*B*Q (AB) or A*Q (BA) are the same for every lambda.  So the loop of
// analyze_regularization.m:22-33 / plot_error_surface.m:28-42 (one solve per lambda) is one Arnoldi
// here; iteration k solves the projected system for every lambda still running and gets all their
// monitors ||b - W_k y_l||, ||V_k y_l - x_true|| and ||V_k y_l|| from two proj_norms passes.
// Column l of every output is what hgm_gmres_bounds_ex(lambda = lambdas[l], hybrid = 1) returns
// (breakdown convention included), entries past niters[l] are NaN.
int gmres_bounds_sweep(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* B, const double* b_in,
                       const double* xt_in, double tol, int maxit, const double* lambdas, int nlam, int side,
                       double* X_out, double* err_surf, double* res_surf, double* sol_surf, int* niters,
                       int* ksteps) {
    check_dims(A, B);
    HGM_REQUIRE(B != nullptr, "B is NULL");
    HGM_REQUIRE(b_in != nullptr, "b is required");
    HGM_REQUIRE(A->dtype == HGM_F64, "lambda sweep: fp64 operators only");
    if (dist_n(c) || c->host_ar != nullptr)
        throw Error{HGM_E_UNSUPPORTED, "lambda sweep: single rank only (no communicator / all-reduce hook)"};
    HGM_REQUIRE(!c->num.parity, "lambda sweep: not in parity mode");
    HGM_REQUIRE(!(o && (o->flags & HGM_DEVICE_PTRS)), "lambda sweep: host buffers only (HGM_DEVICE_PTRS refused)");
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    HGM_REQUIRE(nlam >= 1 && lambdas != nullptr, "lambda sweep: at least one lambda");
    for (int l = 0; l < nlam; ++l)
        HGM_REQUIRE(std::isfinite(lambdas[l]) && lambdas[l] >= 0.0, "lambda sweep: every lambda must be finite and >= 0");
    HGM_REQUIRE(niters != nullptr, "niters is required");
    const PixOrder po = n_order(c, A, B);
    const int orth = o ? o->orth : HGM_MGS;
    const int64_t m = A->rows, n = A->cols;
    const bool nspace = side == HGM_SIDE_BA;
    const int64_t dim = nspace ? n : m;
    const int64_t ldaq = round_up(m > 0 ? m : 1, 64), ldbq = round_up(n > 0 ? n : 1, 64);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const size_t surf = (size_t)maxit * nlam;
    if (err_surf) std::fill(err_surf, err_surf + surf, nan);
    if (res_surf) std::fill(res_surf, res_surf + surf, nan);
    if (sol_surf) std::fill(sol_surf, sol_surf + surf, nan);

    const KrylovBasis kb = krylov_basis(c, "Q", dim, maxit + 1, false);
    double* Q = kb.Q;
    const int64_t ldq = kb.ld;
    // kept products: BA: W = A*Q ; AB: V = B*Q and W = A*B*Q
    double* AQ = nspace ? c->buf<double>("AQ", (size_t)ldaq * maxit) : nullptr;
    double* BQ = nspace ? nullptr : c->buf<double>("BQ", (size_t)ldbq * maxit);
    double* ABQ = nspace ? nullptr : c->buf<double>("ABQ", (size_t)ldaq * maxit);
    const double* V = nspace ? Q : BQ;
    const int64_t ldv = nspace ? ldq : ldbq;
    const double* W = nspace ? AQ : ABQ;
    double* x = c->buf<double>("x", n > 0 ? n : 1);
    double* Hd = c->buf<double>("H", (size_t)(maxit + 1) * maxit);
    const int64_t ldy = maxit;
    double* Yd[2] = {c->buf<double>("sweep_Y0", (size_t)ldy * nlam), c->buf<double>("sweep_Y1", (size_t)ldy * nlam)};
    double* mon = c->buf<double>("sweep_mon", (size_t)4 * nlam);   // [res^2 | (W y)^2 | err^2 | (V y)^2]
    HGM_HIP(hipMemsetAsync(Hd, 0, sizeof(double) * (maxit + 1) * maxit, c->stream));
    const double* b = stage_in<double>(c, "in_b", b_in, m, false);
    const double* xt = stage_in_n<double>(c, "in_xt", xt_in, n, false, po);

    sumsq<double>(c, m, b, dslot<double>(c, S_NB));
    if (xt) sumsq<double>(c, n, xt, dslot<double>(c, S_NXT));
    start_residual(c, B, b, nspace, kb, dslot<double>(c, S_BETA));           // r0 (*_bounds.m:11-13)
    read_scalars(c, 0, 3);
    const double nb = std::sqrt(c->hscal[S_NB]);
    const double nxt = xt ? std::sqrt(c->hscal[S_NXT]) : 0.0;
    const double beta = std::sqrt(c->hscal[S_BETA]);
    div_scalar<double>(c, dim, Q, Q, beta);

    const FusedPlan* fplan = nspace ? nullptr : fused_ab_plan(c, A, B);
    std::vector<double> H((size_t)(maxit + 1) * maxit, 0.0);
    auto Hh = [&](int i, int j) -> double& { return H[(size_t)j * (maxit + 1) + i]; };
    std::vector<char> active(nlam, 1);
    int nactive = nlam;
    std::vector<double> Yh((size_t)ldy * nlam), G, mh((size_t)4 * nlam);
    // lambda l stops with iterate kx (0-based iteration; -1: x never assigned) after nit iterations
    auto finish = [&](int l, int nit, int kx) {
        active[l] = 0;
        --nactive;
        niters[l] = nit;
        if (X_out == nullptr || kx < 0) return;
        gemv<double>(c, n, kx + 1, V, ldv, Yd[kx & 1] + (size_t)l * ldy, x, 0);      // :37-38  x = V_k y
        stage_out_n<double>(c, X_out + (size_t)l * n, x, n, false, po);
    };
    int k = 0;
    bool unassigned = false;
    for (k = 0; k < maxit && nactive > 0; ++k) {
        double* qk = Q + (int64_t)k * ldq;
        double* v = Q + (int64_t)(k + 1) * ldq;
        const double* src = nullptr;                                  // the vector the sweep orthogonalises
        // ---- operator (*_bounds.m:25) ----
        if (nspace) {
            apply_M(c, A, B, nullptr, true, qk, AQ + (int64_t)k * ldaq, v);
        } else {
            double* w = ABQ + (int64_t)k * ldaq;
            apply_M(c, A, B, fplan, false, qk, BQ + (int64_t)k * ldbq, w);
            if (orth == HGM_CGS2)
                HGM_HIP(hipMemcpyAsync(v, w, sizeof(double) * m, hipMemcpyDeviceToDevice, c->stream));
            else src = w;
        }
        // ---- orthogonalisation (:26-32) ----
        double* Hcol = Hd + (int64_t)k * (maxit + 1);
        if (orth == HGM_CGS2) cgs2<double>(c, dim, Q, ldq, k, Hcol, false);
        else mgs<double>(c, dim, Q, ldq, k, Hcol, false, src);
        Reader rd(c);
        rd.add(&Hh(0, k), Hcol, sizeof(double) * (k + 2));
        rd.go();
        if (Hh(k + 1, k) == 0) {                                 // :31  breakdown: every lambda stops here
            if (k == 0) unassigned = true;
            for (int l = 0; l < nlam; ++l)
                if (active[l]) {
                    // the single solver's convention: niters = k + 1, history entry k stays 0, x is
                    // the previous iterate
                    if (err_surf) err_surf[(size_t)l * maxit + k] = 0.0;
                    if (res_surf) res_surf[(size_t)l * maxit + k] = 0.0;
                    if (sol_surf) sol_surf[(size_t)l * maxit + k] = 0.0;
                    finish(l, k + 1, k - 1);
                }
            ++k;
            break;
        }
        // ---- projected solves (:34-36), one per running lambda; Hk'*Hk and Hk'*tk are shared ----
        const int kk = k + 1;
        G.assign((size_t)kk * kk, 0.0);
        dense::normal_matrix(H.data(), maxit + 1, kk, G.data());
        std::fill(Yh.begin(), Yh.end(), 0.0);
        for (int l = 0; l < nlam; ++l)
            if (active[l]) dense::proj_ptr(G.data(), H.data(), maxit + 1, kk, beta, lambdas[l], &Yh[(size_t)l * ldy]);
        double* Yk = Yd[k & 1];
        h2d(c, Yk, Yh.data(), sizeof(double) * Yh.size());
        // ---- monitors of every lambda (:37-41): two passes over the kept products ----
        proj_norms<double>(c, m, kk, W, ldaq, Yk, ldy, nlam, b, mon, mon + nlam);
        proj_norms<double>(c, n, kk, V, ldv, Yk, ldy, nlam, xt, mon + 2 * nlam, mon + 3 * nlam);
        Reader rm(c);
        rm.add(mh.data(), mon, sizeof(double) * 4 * nlam);
        rm.go();
        for (int l = 0; l < nlam; ++l) {
            if (!active[l]) continue;
            const double res = std::sqrt(mh[l]) / nb;
            if (res_surf) res_surf[(size_t)l * maxit + k] = res;
            if (err_surf && xt) err_surf[(size_t)l * maxit + k] = std::sqrt(mh[2 * (size_t)nlam + l]) / nxt;
            if (sol_surf) sol_surf[(size_t)l * maxit + k] = std::sqrt(mh[3 * (size_t)nlam + l]);
            if (res <= tol || kk == maxit) finish(l, kk, k);      // :79-83
        }
    }
    if (ksteps) *ksteps = k;
    if (o && o->H_out) std::memcpy(o->H_out, H.data(), sizeof(double) * H.size());
    if (unassigned)
        throw Error{HGM_E_NOT_ASSIGNED, "Output argument \"x\" not assigned during call (breakdown at k = 1)"};
    return HGM_OK;
}

// ============================================================================
// Batched *_bounds solves: nrhs right-hand sides against one operator pair in lockstep
// ============================================================================
// plot_error_vs_noise_level.m:28-54 runs the four *_bounds solvers for every noise level on the same
// A and B: each of those solves streams the operators from HBM once per iteration.  Here the columns
// advance together and iteration k's operator is two multi-vector passes (spmm.hip) over the packed
// q_k of the columns still running, so the operators' entries are read once per group of up to 8
// columns.  Everything else is the single solver's, per column: one Krylov basis each (one slab, the
// k-th vectors a constant stride apart), mgs / cgs2, the host projected solve (*_bounds.m:34-36), the
// monitors from the kept products (:37-41, recon).  Column j of every output is what
// hgm_gmres_bounds_ex(b = Bm(:,j), x_true = XT(:,j), lambda = lambdas[j]) returns, with its own
// stopping iteration and breakdown convention; a finished column leaves the batch and the later
// passes are repacked over the rest.  The multi-vector product's bits do not depend on the group a
// column is packed into, and every other kernel runs per column with scratch of its own, so a
// column's bits do not depend on its neighbours (which is why even one column takes the spmm route
// and never the one-pass plan).
//
// lockstep_core is that loop; its callers differ in two things (Lockstep):
//  * the column's right-hand side: column j of a matrix (hgm_gmres_bounds_batch) or one b shared by
//    every column (the mismatch sweep);
//  * the B pass: spmm(B) for every column, or the perturbed product (spmm.hip k_spmm_pert) in which
//    column j applies B + coefs[j] * E, the coefficients packed with the running columns as they are
//    regrouped; or, with the matrix-free Gaussian G for E, spmm(B) followed by the accumulating Gaussian
//    product (gauss.hip k_gauss_mm) with the same packed coefficients.  The A pass is spmm(A) either way.
// With arnoldi set it is the GCV Arnoldi of gcv_function.m:3-33 per column instead of a solve: no
// projected solve, no monitors and no kept products; a column leaves at H(k+1,k) < btol (:30) with
// niters[j] = the steps done (hgm_arnoldi's kdone).
namespace {
// The column batch of a lockstep solve (lockstep_core and gk_batch): the right-hand sides, x_true and the
// iterates of nrhs columns as device slabs with a constant column stride, and the way in and out.
struct ColBatch {
    // column j of a slab; one shared column serves every j
    struct Cols {
        double* p = nullptr;
        int64_t ld = 0;
        bool shared = false;
        double* operator()(int j) const { return p + (size_t)ld * (shared ? 0 : j); }
    };
    Cols bj, xtj, xj;
    int nrhs = 0;
    int64_t n = 0;
    PixOrder po;

    // the requirements of the entry points that take column matrices; shared_b: ldb == 0 is one b for every column
    static void require(const std::string& what, const hgm_mat* A, const double* Bm, int64_t ldb, bool shared_b,
                        int nrhs, const double* xt_in, int64_t ldxt, int maxit, const double* X_out, int64_t ldx,
                        const int* niters) {
        HGM_REQUIRE(nrhs >= 1 && nrhs <= 64, what + ": 1 <= nrhs <= 64");
        HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
        HGM_REQUIRE(Bm != nullptr && niters != nullptr, "Bm and niters are required");
        const int64_t m = A->rows, n = A->cols;
        if (shared_b) HGM_REQUIRE(ldb == 0 || ldb >= m, what + ": ldb is 0 (one shared b) or >= rows(A)");
        else HGM_REQUIRE(ldb >= m, what + ": ldb >= rows(A)");
        HGM_REQUIRE(X_out == nullptr || ldx >= n, what + ": ldx >= cols(A)");
        HGM_REQUIRE(xt_in == nullptr || ldxt == 0 || ldxt >= n, what + ": ldxt is 0 (one shared x_true) or >= cols(A)");
    }

    // Empty outputs (histories NaN, niters 0), then b (ldrhs == 0: one shared by every column) and x_true (none,
    // ldxt == 0: one shared, or one per column; given in the reference order, kept in the stored pixel order po)
    // on the device.  Workspace names start with pre.  zero_xt: without an x_true the one column is zeroed.
    ColBatch(hgm_ctx* c, const std::string& pre, const hgm_mat* A, const PixOrder& order, int ncols, const double* rhs,
             int64_t ldrhs, const double* xt_in, int64_t ldxt, bool zero_xt, int maxit,
             std::initializer_list<double*> hists, int* niters)
        : nrhs(ncols), n(A->cols), po(order) {
        const int64_t m = A->rows;
        const int64_t ldm = round_up(m > 0 ? m : 1, 64), ldn = round_up(n > 0 ? n : 1, 64);
        for (double* h : hists)
            if (h) std::fill(h, h + (size_t)maxit * nrhs, std::numeric_limits<double>::quiet_NaN());
        for (int j = 0; j < nrhs; ++j) niters[j] = 0;
        const int nb_cols = ldrhs == 0 ? 1 : nrhs;
        const int nxt_cols = xt_in && ldxt != 0 ? nrhs : 1;
        bj = {c->buf<double>((pre + "ball").c_str(), (size_t)ldm * nb_cols), ldm, nb_cols == 1};
        xtj = {c->buf<double>((pre + "xtall").c_str(), (size_t)ldn * nxt_cols), ldn, nxt_cols == 1};
        xj = {c->buf<double>((pre + "xall").c_str(), (size_t)ldn * nrhs), ldn, false};
        for (int j = 0; j < nb_cols; ++j) h2d(c, bj.p + (size_t)ldm * j, rhs + (size_t)ldrhs * j, sizeof(double) * m);
        if (xt_in) {
            // x_true in the reference order, permuted into the operators' stored pixel order
            double* tmp = po.trivial() ? nullptr : c->buf<double>((pre + "xt_ref").c_str(), n > 0 ? n : 1);
            for (int j = 0; j < nxt_cols; ++j) {
                double* dst = xtj.p + (size_t)ldn * j;
                h2d(c, po.trivial() ? dst : tmp, xt_in + (size_t)ldxt * j, sizeof(double) * n);
                if (!po.trivial()) pix_permute<double>(c, po, tmp, dst, 0);
            }
        } else if (zero_xt) {
            HGM_HIP(hipMemsetAsync(xtj.p, 0, sizeof(double) * ldn, c->stream));
        }
    }

    // the iterates into the columns of X_out, in the reference order (assigned: only the columns it marks)
    void stage_out(hgm_ctx* c, double* X_out, int64_t ldx, const std::vector<char>* assigned = nullptr) const {
        if (!X_out) return;
        for (int j = 0; j < nrhs; ++j)
            if (!assigned || (*assigned)[j]) stage_out_n<double>(c, X_out + (size_t)ldx * j, xj(j), n, false, po);
    }
};

// the operator's entries once and the interleaved vectors once each way
double spmm_bytes(const hgm_mat* M, int nv) { return 12.0 * M->nnz + 8.0 * spmm_width(nv) * (M->rows + M->cols); }

// spmm as a KC_SPMM bracket of its own
void spmm_timed(hgm_ctx* c, const hgm_mat* M, int nv, const double* in, double* out) {
    hipEvent_t tev = nullptr;
    timing_begin(c, KC_SPMM, &tev);
    spmm(c, M, nv, in, out);
    timing_end(c, KC_SPMM, tev, spmm_bytes(M, nv));
}

struct Lockstep {
    const double* rhs = nullptr;         // column j's right-hand side: rhs + ldrhs * j (host)
    int64_t ldrhs = 0;                   // 0: one b shared by every column
    Perturbation P;                      // the B pass: spmm(B) (none), the perturbed product (P.E), or spmm(B)
                                         // then + c_j G (P.G, gauss.hip); c_j = P.coefs[j]
    bool arnoldi = false;
    double btol = 0.0;                   // arnoldi: the break threshold
    double* beta_out = nullptr;          // arnoldi: ||r0|| per column
};

int lockstep_core(hgm_ctx* c, const Lockstep& L, int orth, double* H_out, const hgm_mat* A, const hgm_mat* B,
                  int nrhs, const double* xt_in, int64_t ldxt, double tol, int maxit, const double* lambdas, int side,
                  int hybrid, double* X_out, int64_t ldx, double* err_hist, double* res_hist, int* niters,
                  int* col_status) {
    const int64_t m = A->rows, n = A->cols;
    const bool pert = L.P.E != nullptr;
    // E on B's pattern: one compare pass over the index streams per solve
    const bool pert_shared = pert && c->num.pert_shared && same_pattern(c, B, L.P.E);
    const bool nspace = side == HGM_SIDE_BA;
    const int64_t dim = nspace ? n : m;
    const int64_t ldm = round_up(m > 0 ? m : 1, 64), ldn = round_up(n > 0 ? n : 1, 64);
    const size_t hs = (size_t)(maxit + 1) * maxit;           // one column's Hessenberg
    // (the monitor reads x_true's column also without an x_true, so that one is zeroed: errors stay NaN)
    const ColBatch cb(c, "bt_", A, n_order(c, A, B), nrhs, L.rhs, L.ldrhs, xt_in, ldxt, true, maxit,
                      {err_hist, res_hist}, niters);
    const ColBatch::Cols &bj = cb.bj, &xtj = cb.xtj, &xj = cb.xj;
    if (col_status) std::fill(col_status, col_status + nrhs, (int)HGM_OK);

    // ---- device storage: every per-column array is one slab with a constant column stride ----
    const KrylovBasis kb = krylov_basis(c, "bt_Q", dim, (maxit + 1) * nrhs, false);
    double* Qall = kb.Q;
    const int64_t ldq = kb.ld;
    const size_t qs = (size_t)ldq * (maxit + 1);            // one column's basis
    // kept products: BA: W = A*Q ; AB: V = B*Q and W = A*B*Q  (the sweep's, per column).  The Arnoldi
    // keeps none: AB needs the current A*B*q alone (one vector per column), BA nothing.
    const int kept = L.arnoldi ? 1 : maxit;
    auto kslot = [&](int k) { return L.arnoldi ? 0 : k; };
    double* Wall = c->buf<double>("bt_W", (size_t)ldm * kept * nrhs);
    double* Vall = nspace || L.arnoldi ? nullptr : c->buf<double>("bt_V", (size_t)ldn * kept * nrhs);
    double* Hd = c->buf<double>("bt_H", hs * nrhs);
    double* Yd = c->buf<double>("bt_y", (size_t)maxit * nrhs);
    double* mon = c->buf<double>("bt_mon", (size_t)2 * nrhs);          // [res^2, err^2] per column
    double* scal = c->buf<double>("bt_scal", (size_t)3 * nrhs);        // [||b||^2, ||x_true||^2, ||r0||^2] per column
    // interleaved multi-vectors of the operator passes (two per space: source and product)
    double* Im[2] = {c->buf<double>("bt_im0", (size_t)(m > 0 ? m : 1) * SPMM_MAXV),
                c->buf<double>("bt_im1", (size_t)(m > 0 ? m : 1) * SPMM_MAXV)};
    double* In[2] = {c->buf<double>("bt_in0", (size_t)(n > 0 ? n : 1) * SPMM_MAXV),
                c->buf<double>("bt_in1", (size_t)(n > 0 ? n : 1) * SPMM_MAXV)};
    HGM_HIP(hipMemsetAsync(Hd, 0, sizeof(double) * hs * nrhs, c->stream));
    auto Qj = [&](int j) { return Qall + qs * (size_t)j; };
    auto Wj = [&](int j) { return Wall + (size_t)ldm * kept * j; };
    auto Vj = [&](int j) -> const double* { return nspace ? Qj(j) : Vall + (size_t)ldn * kept * j; };
    const int64_t ldv = nspace ? ldq : ldn;

    // per-column scratch of the orthogonalisation: the one-reduction MGS keeps its Gram triangle in a
    // workspace buffer from step to step, so every column gets workspace names of its own
    struct ColTag {
        hgm_ctx* c;
        std::string saved;
        ColTag(hgm_ctx* cc, int j) : c(cc), saved(cc->ws_tag) { c->ws_tag = "bt" + std::to_string(j) + ":"; }
        ~ColTag() { c->ws_tag = saved; }
    };
    // one operator pass pair over the columns `cols` (at most 8): src(j) -> [mid(j)] -> dst(j)
    auto operator_pass = [&](const std::vector<int>& cols, size_t g0, int nv, const hgm_mat* first,
                             const hgm_mat* second, auto src, auto mid, auto dst) {
        MvCols ts, tm, td;
        double cf[SPMM_MAXV];                                    // the group's coefficients, packed as its columns
        for (int r = 0; r < SPMM_MAXV; ++r) {
            ts.p[r] = tm.p[r] = td.p[r] = nullptr;
            cf[r] = 0.0;
        }
        for (int r = 0; r < nv; ++r) {
            const int j = cols[g0 + r];
            ts.p[r] = const_cast<double*>(src(j));
            tm.p[r] = mid(j);
            td.p[r] = dst(j);
            if (pert || L.P.G) cf[r] = L.P.coefs[j];
        }
        double bytes = 0.0;
        // one pass of the pair: spmm(A), and for B either spmm(B) or the perturbed product
        auto product = [&](const hgm_mat* M, const double* in, double* out) {
            if (M == B && pert) {
                spmm_pert(c, B, L.P.E, pert_shared, nv, cf, in, out);
                bytes += (pert_shared ? 20.0 * B->nnz : 12.0 * ((double)B->nnz + L.P.E->nnz)) +
                         8.0 * spmm_width(nv) * (M->rows + M->cols);
            } else {
                spmm(c, M, nv, in, out);   // (inside this pass's one KC_SPMM bracket, so not spmm_timed)
                bytes += spmm_bytes(M, nv);
                // out = (B in) + (c_j * (G in)), G in the reference row order whatever B's stored one is
                if (M == B && L.P.G) gauss_mm(c, L.P.G, B->row_order, nv, cf, true, in, out);
            }
        };
        hipEvent_t tev = nullptr;
        timing_begin(c, KC_SPMM, &tev);
        // first: cols(first) -> rows(first) ; second: rows(first) = cols(second) -> rows(second)
        const bool from_m = first == B;                          // B maps the ray space to the pixel space
        double* I0 = from_m ? Im[0] : In[0];
        double* I1 = from_m ? In[0] : Im[0];
        mv_pack(c, first->cols, nv, ts, I0);
        product(first, I0, I1);
        if (tm.p[0]) mv_unpack(c, first->rows, nv, I1, tm);
        if (second) {
            double* I2 = from_m ? Im[1] : In[1];
            product(second, I1, I2);
            mv_unpack(c, second->rows, nv, I2, td);
        }
        timing_end(c, KC_SPMM, tev, bytes);
    };

    // ---- r0 (*_bounds.m:11-13): BA: B*(b - A*0) ; AB: b - A*(B*0) ----
    std::vector<int> act(nrhs);
    for (int j = 0; j < nrhs; ++j) act[j] = j;
    if (nspace) {
        for (size_t g0 = 0; g0 < act.size(); g0 += SPMM_MAXV) {
            const int nv = (int)std::min<size_t>(SPMM_MAXV, act.size() - g0);
            operator_pass(act, g0, nv, B, nullptr, [&](int j) { return (const double*)bj(j); },
                          [&](int j) { return Qj(j); }, [&](int) { return (double*)nullptr; });
        }
    } else {
        for (int j = 0; j < nrhs; ++j)
            HGM_HIP(hipMemcpyAsync(Qj(j), bj(j), sizeof(double) * m, hipMemcpyDeviceToDevice, c->stream));
    }
    for (int j = 0; j < nrhs; ++j) {
        sumsq<double>(c, m, bj(j), scal + 3 * j);
        if (xt_in) sumsq<double>(c, n, xtj(j), scal + 3 * j + 1);
        sumsq<double>(c, dim, Qj(j), scal + 3 * j + 2);
    }
    std::vector<double> sh((size_t)3 * nrhs, 0.0);
    {
        Reader rd(c);
        rd.add(sh.data(), scal, sizeof(double) * 3 * nrhs);
        rd.go();
    }
    std::vector<double> nb(nrhs), nxt(nrhs), beta(nrhs);
    for (int j = 0; j < nrhs; ++j) {
        nb[j] = std::sqrt(sh[3 * (size_t)j]);
        nxt[j] = xt_in ? std::sqrt(sh[3 * (size_t)j + 1]) : 0.0;
        beta[j] = std::sqrt(sh[3 * (size_t)j + 2]);
        div_scalar<double>(c, dim, Qj(j), Qj(j), beta[j]);      // :13  Q(:,1) = r0 / beta
    }

    std::vector<double> H(hs * nrhs, 0.0);
    auto Hh = [&](int j, int i, int k) -> double& { return H[hs * (size_t)j + (size_t)k * (maxit + 1) + i]; };
    std::vector<char> x_assigned(nrhs, 0);
    std::vector<double> Yh((size_t)maxit * nrhs, 0.0), mh((size_t)2 * nrhs, 0.0), M;
    std::vector<int> next, ran;
    bool unassigned = false;
    for (int k = 0; k < maxit && !act.empty(); ++k) {
        // ---- operator (*_bounds.m:25) over the running columns, repacked in groups of at most 8 ----
        for (size_t g0 = 0; g0 < act.size(); g0 += SPMM_MAXV) {
            const int nv = (int)std::min<size_t>(SPMM_MAXV, act.size() - g0);
            auto qk = [&](int j) { return (const double*)(Qj(j) + (int64_t)k * ldq); };
            if (nspace)    // A*q kept, B*(A*q) is the new basis vector
                operator_pass(act, g0, nv, A, B, qk,
                              [&](int j) { return L.arnoldi ? (double*)nullptr : Wj(j) + (int64_t)k * ldm; },
                              [&](int j) { return Qj(j) + (int64_t)(k + 1) * ldq; });
            else           // B*q and A*(B*q) kept; the latter is orthogonalised into the new basis vector
                operator_pass(act, g0, nv, B, A, qk,
                              [&](int j) {
                                  return L.arnoldi ? (double*)nullptr : const_cast<double*>(Vj(j)) + (int64_t)k * ldn;
                              },
                              [&](int j) { return Wj(j) + (int64_t)kslot(k) * ldm; });
        }
        // ---- orthogonalisation (:26-32), the single solver's sweep once per running column ----
        for (int j : act) {
            ColTag tag(c, j);
            double* Q = Qj(j);
            double* v = Q + (int64_t)(k + 1) * ldq;
            const double* src = nullptr;
            if (!nspace) {
                const double* w = Wj(j) + (int64_t)kslot(k) * ldm;
                if (orth == HGM_CGS2)
                    HGM_HIP(hipMemcpyAsync(v, w, sizeof(double) * m, hipMemcpyDeviceToDevice, c->stream));
                else src = w;
            }
            double* Hcol = Hd + hs * (size_t)j + (size_t)k * (maxit + 1);
            if (orth == HGM_CGS2) cgs2<double>(c, dim, Q, ldq, k, Hcol, false);
            else mgs<double>(c, dim, Q, ldq, k, Hcol, false, src);
        }
        {
            Reader rd(c);
            for (int j : act)
                rd.add(&Hh(j, 0, k), Hd + hs * (size_t)j + (size_t)k * (maxit + 1), sizeof(double) * (k + 2));
            rd.go();
        }
        // ---- projected solves (:34-36) on the host, per column ----
        const int kk = k + 1;
        next.clear();
        ran.clear();
        if (L.arnoldi) {
            // gcv_function.m:30: the step counts, and the column breaks before Q(:,k+1) = v / H(k+1,k)
            for (int j : act) {
                niters[j] = kk;
                if (!(Hh(j, k + 1, k) < L.btol)) next.push_back(j);
            }
            act.swap(next);
            continue;
        }
        for (int j : act) {
            if (Hh(j, k + 1, k) == 0) {                          // :31  breakdown of this column
                // the single solver's convention: niters = k + 1, history entry k stays 0, x is the
                // previous iterate (never assigned at k = 1)
                if (err_hist) err_hist[(size_t)j * maxit + k] = 0.0;
                if (res_hist) res_hist[(size_t)j * maxit + k] = 0.0;
                niters[j] = k + 1;
                if (k == 0) {
                    unassigned = true;
                    if (col_status) col_status[j] = HGM_E_NOT_ASSIGNED;
                }
                continue;
            }
            const double* Hj = &Hh(j, 0, 0);
            double* y = &Yh[(size_t)j * maxit];
            if (!hybrid) {
                dense::proj_ls(Hj, maxit + 1, kk, beta[j], y);
            } else {
                M.assign((size_t)kk * kk, 0.0);
                dense::normal_matrix(Hj, maxit + 1, kk, M.data());
                dense::proj_ptr(M.data(), Hj, maxit + 1, kk, beta[j], lambdas[j], y);
            }
            ran.push_back(j);
        }
        // ---- monitors (:37-41) from the kept products: x = V_k y, ||x - x_true||^2, ||b - W_k y||^2 ----
        if (!ran.empty()) {
            h2d(c, Yd, Yh.data(), sizeof(double) * Yh.size());
            for (int j : ran) {
                recon<double>(c, n, kk, Vj(j), ldv, Yd + (size_t)j * maxit, xj(j), xtj(j), mon + 2 * j + 1, m, Wj(j),
                              ldm, bj(j), mon + 2 * j);
                x_assigned[j] = 1;
            }
            Reader rm(c);
            rm.add(mh.data(), mon, sizeof(double) * 2 * nrhs);
            rm.go();
        }
        for (int j : ran) {
            const double res = std::sqrt(mh[2 * (size_t)j]) / nb[j];
            if (res_hist) res_hist[(size_t)j * maxit + k] = res;
            if (err_hist && xt_in) err_hist[(size_t)j * maxit + k] = std::sqrt(mh[2 * (size_t)j + 1]) / nxt[j];
            if (res <= tol || kk == maxit) niters[j] = kk;        // :79-83  this column leaves the batch
            else next.push_back(j);
        }
        act.swap(next);
    }
    cb.stage_out(c, X_out, ldx, &x_assigned);
    if (H_out) std::memcpy(H_out, H.data(), sizeof(double) * H.size());
    if (L.beta_out) std::copy(beta.begin(), beta.end(), L.beta_out);
    if (unassigned)
        throw Error{HGM_E_NOT_ASSIGNED, "Output argument \"x\" not assigned in at least one column (breakdown at k = 1)"};
    return HGM_OK;
}

// the refusals every lockstep entry point shares
void lockstep_guard(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* B, const std::string& what) {
    check_dims(A, B);
    HGM_REQUIRE(B != nullptr, "B is NULL");
    HGM_REQUIRE(A->dtype == HGM_F64, what + ": fp64 operators only");
    if (dist_n(c) || c->host_ar != nullptr)
        throw Error{HGM_E_UNSUPPORTED, what + ": single rank only (no communicator / all-reduce hook)"};
    HGM_REQUIRE(!c->num.parity, what + ": not in parity mode");
    HGM_REQUIRE(!(o && (o->flags & HGM_DEVICE_PTRS)), what + ": host buffers only (HGM_DEVICE_PTRS refused)");
}

void lockstep_lambdas(const double* lambdas, int ncols, int hybrid, const std::string& what) {
    if (!hybrid) return;
    HGM_REQUIRE(lambdas != nullptr, what + ": lambdas are required with hybrid = 1");
    for (int j = 0; j < ncols; ++j)
        HGM_REQUIRE(std::isfinite(lambdas[j]) && lambdas[j] >= 0.0, what + ": every lambda must be finite and >= 0");
}

// the perturbation of a mismatch sweep (E or the Gaussian G, and the coefficients) against its B0
void mismatch_guard(const hgm_mat* A, const hgm_mat* B0, const Perturbation& P, const std::string& what) {
    if (P.G) {
        HGM_REQUIRE(A != B0, what + ": A and B0 must be distinct operators");
        HGM_REQUIRE(P.G->rows == B0->rows && P.G->cols == B0->cols, what + ": G must have B0's shape");
        HGM_REQUIRE(B0->col_order.trivial(), what + ": B0's columns must be in the reference order");
    } else {
        const hgm_mat* E = P.E;
        HGM_REQUIRE(E != nullptr, what + ": E is NULL");
        HGM_REQUIRE(E->dtype == HGM_F64, what + ": fp64 operators only");
        HGM_REQUIRE(A != B0 && E != A, what + ": A, B0 and E must be distinct operators");
        HGM_REQUIRE(E->rows == B0->rows && E->cols == B0->cols, what + ": E must have B0's shape");
        HGM_REQUIRE(E->row_order == B0->row_order && E->col_order == B0->col_order,
                    what + ": E must be stored in B0's row and column order");
    }
    HGM_REQUIRE(P.ncoef >= 1 && P.ncoef <= 64, what + ": 1 <= ncoef <= 64");
    HGM_REQUIRE(P.coefs != nullptr, what + ": coefs is required");
    for (int j = 0; j < P.ncoef; ++j)
        HGM_REQUIRE(std::isfinite(P.coefs[j]), what + ": every coefficient must be finite");
}
}  // namespace

int gmres_bounds_batch(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* B, const double* Bm,
                       int64_t ldb, int nrhs, const double* xt_in, int64_t ldxt, double tol, int maxit,
                       const double* lambdas, int side, int hybrid, double* X_out, int64_t ldx, double* err_hist,
                       double* res_hist, int* niters, int* col_status) {
    const std::string what = "batched solve";
    lockstep_guard(c, o, A, B, what);
    ColBatch::require(what, A, Bm, ldb, false, nrhs, xt_in, ldxt, maxit, X_out, ldx, niters);
    lockstep_lambdas(lambdas, nrhs, hybrid, what);
    Lockstep L;
    L.rhs = Bm;
    L.ldrhs = ldb > 0 ? ldb : 1;                              // never 0 (one shared b), also with m == 0
    return lockstep_core(c, L, o ? o->orth : HGM_MGS, o ? o->H_out : nullptr, A, B, nrhs, xt_in, ldxt, tol, maxit,
                         lambdas, side, hybrid, X_out, ldx, err_hist, res_hist, niters, col_status);
}

// plot_error_vs_mismatch_norm.m:23-61 / run_2D_phantom.m:79-102: column j is the *_bounds solve of the
// one b with the back-projector B0 + coefs[j] * E.  No such operator is formed: B0 and E are read once
// per group of up to 8 running levels (spmm.hip k_spmm_pert); with the matrix-free dense Gaussian G for E
// (plot_error_vs_mismatch_norm.m:16-17: E = randn(size(A'))) nothing of G is stored, the B pass regenerates
// it (gauss.hip).
int gmres_bounds_mismatch(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* B0, const Perturbation& P,
                          const double* b, const double* xt_in, double tol, int maxit, const double* lambdas, int side,
                          int hybrid, double* X_out, int64_t ldx, double* err_hist, double* res_hist, int* niters,
                          int* col_status) {
    const std::string what = P.G ? "Gaussian mismatch sweep" : "mismatch sweep";
    lockstep_guard(c, o, A, B0, what);
    mismatch_guard(A, B0, P, what);
    HGM_REQUIRE(maxit >= 1, "maxit must be >= 1");
    HGM_REQUIRE(b != nullptr && niters != nullptr, "b and niters are required");
    HGM_REQUIRE(X_out == nullptr || ldx >= A->cols, what + ": ldx >= cols(A)");
    lockstep_lambdas(lambdas, P.ncoef, hybrid, what);
    Lockstep L;
    L.rhs = b;
    L.P = P;
    return lockstep_core(c, L, o ? o->orth : HGM_MGS, o ? o->H_out : nullptr, A, B0, P.ncoef, xt_in, 0, tol, maxit,
                         lambdas, side, hybrid, X_out, ldx, err_hist, res_hist, niters, col_status);
}

// gcv_function.m:3-33 for every level of a mismatch sweep in lockstep (the two GCV Arnoldis of
// plot_error_vs_mismatch_norm.m:46-50): H holds ncoef consecutive (k+1) x k blocks.
int arnoldi_mismatch(hgm_ctx* c, const hgm_mat* A, const hgm_mat* B0, const Perturbation& P, const double* b, int kg,
                     int side, double btol, int orth, double* H_out, double* beta_out, int* kdone) {
    const std::string what = P.G ? "Gaussian mismatch Arnoldi" : "mismatch Arnoldi";
    lockstep_guard(c, nullptr, A, B0, what);
    mismatch_guard(A, B0, P, what);
    HGM_REQUIRE(kg >= 1, "k must be >= 1");
    HGM_REQUIRE(b != nullptr, "b is required");
    std::vector<int> done(P.ncoef, 0);
    Lockstep L;
    L.rhs = b;
    L.P = P;
    L.arnoldi = true;
    L.btol = btol;
    L.beta_out = beta_out;
    const int st = lockstep_core(c, L, orth, H_out, A, B0, P.ncoef, nullptr, 0, 0.0, kg, nullptr, side, 0, nullptr, 0,
                                 nullptr, nullptr, done.data(), nullptr);
    if (kdone) std::copy(done.begin(), done.end(), kdone);
    return st;
}

// ============================================================================
// Lockstep Golub-Kahan solves (hgm_gk_batch)
// ============================================================================
// lsqr_solver.m, hybrid_lsqr_solver.m, lsmr_solver.m or hybrid_lsmr_solver.m for nrhs columns
// (b_j, x_true_j, lambda_j) in lockstep.  Every state vector (u, v, x, w / h, hbar, the hybrid's lower
// block u_n, and b and x_true themselves) lives in spmm.hip's interleaved layout for the whole solve, in
// groups of up to 8 running columns: spmm(A) and spmm(At) read each operator once per group and pass,
// straight on that state, and the recurrences are gkmv.hip's per-slot kernels.  Packs and unpacks happen
// only at entry, when a column leaves (its x), and for hybrid LSMR's basis column and x = V_k y.  The
// scalars (beta^2, alpha^2, the monitors) of all running columns come back in one transfer each, at
// most three per iteration; the rotations (lsqr_rotate / lsmr_rotate) and the projected solve of hybrid
// LSMR run on the host per column.  A column that stops has its x extracted at that iteration; when the
// running columns then fit narrower groups they are re-gathered (mv_regather).  No kernel's result for
// a slot depends on the group's width, the slot or the other slots, so a column's bits do not depend
// on its neighbours.
namespace {
// one interleaved state vector of the batch: group g at p + g * max(len, 1) * SPMM_MAXV
struct GkVec {
    double* p = nullptr;
    int64_t len = 0;
    double* at(size_t g) const { return p + g * (size_t)(len > 0 ? len : 1) * SPMM_MAXV; }
};
}  // namespace

int gk_batch(hgm_ctx* c, const hgm_opts* o, const hgm_mat* A, const hgm_mat* At, const double* Bm, int64_t ldb,
             int nrhs, const double* xt_in, int64_t ldxt, double tol, int maxit, const double* lambdas, int kind,
             int hybrid, double* X_out, int64_t ldx, double* err_hist, double* res_hist, double* ar_hist, int* niters) {
    const std::string what = "Golub-Kahan batch";
    lockstep_guard(c, o, A, At, what);
    HGM_REQUIRE(kind == HGM_GK_LSQR || kind == HGM_GK_LSMR, what + ": kind is HGM_GK_LSQR or HGM_GK_LSMR");
    ColBatch::require(what, A, Bm, ldb, true, nrhs, xt_in, ldxt, maxit, X_out, ldx, niters);
    lockstep_lambdas(lambdas, nrhs, hybrid, what);
    const int64_t m = A->rows, n = A->cols;
    const bool lsmr = kind == HGM_GK_LSMR, hyb = hybrid != 0;
    const bool hlsqr = !lsmr && hyb, plsmr = lsmr && !hyb, hlsmr = lsmr && hyb;
    const int64_t ldn = round_up(n > 0 ? n : 1, 64);
    const ColBatch cb(c, "gk_", A, n_order(c, A, At), nrhs, Bm, ldb, xt_in, ldxt, false, maxit,
                      {err_hist, res_hist, ar_hist}, niters);
    const ColBatch::Cols &bj = cb.bj, &xtj = cb.xtj, &xj = cb.xj;
    double* const xtall = xtj.p;

    // ---- device storage ----
    const size_t G0 = (size_t)(nrhs + SPMM_MAXV - 1) / SPMM_MAXV;
    auto vec = [&](const char* name, int64_t len) {
        GkVec v;
        v.len = len;
        v.p = c->buf<double>(name, G0 * (size_t)(len > 0 ? len : 1) * SPMM_MAXV);
        return v;
    };
    const bool xt_cols = xt_in && ldxt != 0;                 // else one x_true shared by every column (or none)
    GkVec U = vec("gk_u", m), Bi = vec("gk_b", m), V = vec("gk_v", n), X = vec("gk_x", n);
    GkVec W, H, HB, UN, XT;
    if (!lsmr) W = vec("gk_w", n);
    if (plsmr) {
        H = vec("gk_h", n);
        HB = vec("gk_hbar", n);
    }
    if (hlsqr) UN = vec("gk_un", n);                         // lower block of u_aug (hybrid_lsqr_solver.m:6)
    if (xt_cols) XT = vec("gk_xt", n);
    GkVec tmp_m = vec("gk_tmp_m", m), tmp_n = vec("gk_tmp_n", n);   // re-gather targets
    double* Tm = c->buf<double>("gk_tm", (size_t)(m > 0 ? m : 1) * SPMM_MAXV);   // one group's product
    double* Tn = c->buf<double>("gk_tn", (size_t)(n > 0 ? n : 1) * SPMM_MAXV);
    double* dump = c->buf<double>("gk_dump", (size_t)ldn);   // where the slots of finished columns unpack to
    double* Vall = hlsmr ? c->buf<double>("gk_V", (size_t)ldn * maxit * nrhs) : nullptr;   // per-column bases V_j
    double* Yd = hlsmr ? c->buf<double>("gk_y", (size_t)maxit * nrhs) : nullptr;
    double* dsum = c->buf<double>("gk_sums", 3 * G0 * SPMM_MAXV);
    std::vector<double> hsum(3 * G0 * SPMM_MAXV, 0.0);
    auto ds = [&](int q, size_t g) { return dsum + ((size_t)q * G0 + g) * SPMM_MAXV; };
    auto hs = [&](int q, size_t g, size_t r) { return hsum[((size_t)q * G0 + g) * SPMM_MAXV + r]; };
    auto readback = [&](int nq) {                            // the sums of every running column, one transfer
        Reader rd(c);
        rd.add(hsum.data(), dsum, sizeof(double) * (size_t)nq * G0 * SPMM_MAXV);
        rd.go();
    };
    auto Vj = [&](int j) { return Vall + (size_t)ldn * maxit * j; };

    const int errmode = !xt_in ? MVS_NONE : xt_cols ? MVS_DIFF : MVS_DIFF_SHARED;

    // ---- the running columns, in groups of at most 8: slot -> column, -1 once the column has left ----
    std::vector<std::vector<int>> groups(G0);
    for (int j = 0; j < nrhs; ++j) groups[j / SPMM_MAXV].push_back(j);
    auto ptrs = [&](const std::vector<int>& g, auto colptr, double* dead) {
        MvCols t;
        for (size_t r = 0; r < (size_t)SPMM_MAXV; ++r)
            t.p[r] = r < g.size() ? (g[r] >= 0 ? colptr(g[r]) : dead) : nullptr;
        return t;
    };
    auto coef = [&](const std::vector<int>& g, double dead, auto f) {
        MvCoef k;
        for (size_t r = 0; r < (size_t)SPMM_MAXV; ++r) k.c[r] = r < g.size() && g[r] >= 0 ? (double)f(g[r]) : dead;
        return k;
    };
    auto product = [&](const hgm_mat* M, int nv, const double* in, double* out) { spmm_timed(c, M, nv, in, out); };
    // a launch (or a few) of the interleaved vector kernels over nvecs multi-vectors of length len
    auto vk = [&](int64_t len, int nv, int nvecs, auto&& fn) {
        hipEvent_t tev = nullptr;
        timing_begin(c, KC_GKMV, &tev);
        fn();
        timing_end(c, KC_GKMV, tev, 8.0 * spmm_width(nv) * (double)len * nvecs);
    };
    // Out = (a X) + (b Y) [+ (cz Z)] over one group, with per-slot sums of squares into sums
    auto lin = [&](int64_t len, int nv, int nterms, const double* Xp, const MvCoef& a, const double* Yp,
                   const MvCoef& b, const double* Zp, const MvCoef& cz, double* Out, int sum, const double* D,
                   double* sums) {
        MvLin L;
        L.nterms = nterms;
        L.X = Xp;
        L.Y = Yp;
        L.Z = Zp;
        L.a = a;
        L.b = b;
        L.c = cz;
        L.Out = Out;
        L.sum = sum;
        L.D = D;
        L.sums = sums;
        vk(len, nv, nterms + (Out ? 1 : 0) + (sum == MVS_DIFF ? 1 : 0), [&] { mv_lin(c, len, nv, L); });
    };
    const double* xt_shared = errmode == MVS_DIFF_SHARED ? xtall : nullptr;
    auto errD = [&](size_t g) -> const double* { return errmode == MVS_DIFF ? XT.at(g) : xt_shared; };
    auto copy_group = [&](double* dst, const double* src, int64_t len, int nv) {
        if (len > 0)
            HGM_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)len * spmm_width(nv), hipMemcpyDeviceToDevice,
                                   c->stream));
    };
    auto zero_group = [&](double* dst, int64_t len, int nv) {
        if (len > 0) HGM_HIP(hipMemsetAsync(dst, 0, sizeof(double) * (size_t)len * spmm_width(nv), c->stream));
    };
    MvCoef ones, minus1, none{};
    for (int r = 0; r < SPMM_MAXV; ++r) {
        ones.c[r] = 1.0;
        minus1.c[r] = -1.0;
    }

    // ---- per-column scalars (host, double) ----
    std::vector<double> nb(nrhs), nxt(nrhs, 0.0), beta(nrhs), alpha(nrhs), sq(nrhs, 0.0);
    std::vector<double> rho_bar(nrhs), phi_bar(nrhs), c_x(nrhs, 0.0), c_w(nrhs, 0.0);       // LSQR
    std::vector<double> rot((size_t)9 * nrhs, 0.0), cf((size_t)3 * nrhs, 0.0);              // LSMR (lsmr_rotate)
    const size_t bks = (size_t)(maxit + 1) * maxit;
    std::vector<double> Bk(hlsmr ? bks * nrhs : 0, 0.0), Yh(hlsmr ? (size_t)maxit * nrhs : 0, 0.0);   // hybrid LSMR :11
    std::vector<double> beta1(nrhs, 0.0);
    std::vector<char> stop(nrhs, 0);
    if (hyb)
        for (int j = 0; j < nrhs; ++j) sq[j] = std::sqrt(lambdas[j]);
    double normA = A->fro;                                    // ||A||_F (lsmr_solver.m:71), cached per operator
    if (plsmr && A->fro < 0) {
        double* f = reinterpret_cast<double*>(c->dscal) + 64;
        fro2<double>(c, A, f);
        normA = std::sqrt(read1<double>(c, f));
        const_cast<hgm_mat*>(A)->fro = normA;
    }

    // ---- start: ||b||, ||x_true||, u = b / beta, v = A'u / alpha ----
    if (errmode == MVS_DIFF_SHARED)   // one x_true: its norm from the same kernel a slot of XT would take
        lin(n, 1, 1, xtall, ones, nullptr, none, nullptr, none, nullptr, MVS_SQ, nullptr, ds(2, 0));
    for (size_t g = 0; g < groups.size(); ++g) {
        const int nv = (int)groups[g].size();
        vk(m, nv, 2, [&] { mv_pack(c, m, nv, ptrs(groups[g], bj, nullptr), Bi.at(g)); });
        if (xt_cols) vk(n, nv, 2, [&] { mv_pack(c, n, nv, ptrs(groups[g], xtj, nullptr), XT.at(g)); });
        lin(m, nv, 1, Bi.at(g), ones, nullptr, none, nullptr, none, U.at(g), MVS_SQ, nullptr, ds(0, g));   // u = b, ||b||^2
        if (xt_cols) lin(n, nv, 1, XT.at(g), ones, nullptr, none, nullptr, none, nullptr, MVS_SQ, nullptr, ds(1, g));
        zero_group(X.at(g), n, nv);                                            // x = 0
        if (plsmr) zero_group(HB.at(g), n, nv);                                // lsmr_solver.m:26
        if (hlsqr) zero_group(UN.at(g), n, nv);                                // u_aug = [b; 0] / beta
    }
    readback(3);
    for (size_t g = 0; g < groups.size(); ++g)
        for (size_t r = 0; r < groups[g].size(); ++r) {
            const int j = groups[g][r];
            nb[j] = std::sqrt(hs(0, g, r));
            if (xt_in) nxt[j] = std::sqrt(xt_cols ? hs(1, g, r) : hs(2, 0, 0));
            beta[j] = beta1[j] = nb[j];                                        // lsqr :7, lsmr :11, hybrid lsmr :7
        }
    for (size_t g = 0; g < groups.size(); ++g) {
        const int nv = (int)groups[g].size();
        const auto& G = groups[g];
        // lsqr :8 / hybrid lsmr :8 u = b / beta ; lsmr :12 only where beta > 0
        vk(m, nv, 2, [&] { mv_div(c, m, nv, U.at(g), U.at(g), coef(G, 1.0, [&](int j) { return beta[j]; }), plsmr); });
        product(At, nv, U.at(g), V.at(g));                                     // v_hat = A'*u
        if (hlsqr)   // A_aug'*u_aug = A'*u + sqrt(lambda)*u_n
            lin(n, nv, 2, V.at(g), ones, UN.at(g), coef(G, 0.0, [&](int j) { return sq[j]; }), nullptr, none, V.at(g),
                MVS_SQ, nullptr, ds(0, g));
        else
            lin(n, nv, 1, V.at(g), ones, nullptr, none, nullptr, none, nullptr, MVS_SQ, nullptr, ds(0, g));
    }
    readback(1);
    for (size_t g = 0; g < groups.size(); ++g) {
        const int nv = (int)groups[g].size();
        const auto& G = groups[g];
        for (size_t r = 0; r < G.size(); ++r) {
            const int j = G[r];
            alpha[j] = std::sqrt(hs(0, g, r));                                 // lsqr :11, lsmr :15, hybrid lsmr :14
            rho_bar[j] = alpha[j];                                             // lsqr :15-16
            phi_bar[j] = beta[j];
            // lsmr_rotate's state: [alpha, alphabar, rho, rhobar, cbar, sbar, zetabar = alpha*beta (:19-23), 0, -]
            const double r0[9] = {alpha[j], alpha[j], 1, 1, 1, 0, alpha[j] * beta[j], 0.0, 0.0};
            std::copy(r0, r0 + 9, &rot[(size_t)9 * j]);
        }
        vk(n, nv, 2, [&] { mv_div(c, n, nv, V.at(g), V.at(g), coef(G, 1.0, [&](int j) { return alpha[j]; }), plsmr); });
        if (!lsmr) copy_group(W.at(g), V.at(g), n, nv);                        // lsqr :14 w = v
        if (plsmr) copy_group(H.at(g), V.at(g), n, nv);                        // lsmr :25 h = v
        if (hlsmr)                                                             // hybrid lsmr :15-16 V(:,1)
            vk(n, nv, 2, [&] { mv_unpack(c, n, nv, V.at(g), ptrs(G, [&](int j) { return Vj(j); }, dump)); });
    }

    // the running columns compacted into groups of 8 when that narrows a group or drops one
    auto regather = [&]() {
        std::vector<std::pair<size_t, size_t>> live;
        size_t old_w = 0;
        for (size_t g = 0; g < groups.size(); ++g) {
            old_w += (size_t)spmm_width((int)groups[g].size());
            for (size_t r = 0; r < groups[g].size(); ++r)
                if (groups[g][r] >= 0) live.push_back({g, r});
        }
        const size_t ng = (live.size() + SPMM_MAXV - 1) / SPMM_MAXV;
        size_t new_w = 0;
        for (size_t g = 0; g < ng; ++g) new_w += (size_t)spmm_width((int)std::min<size_t>(SPMM_MAXV, live.size() - g * SPMM_MAXV));
        if (new_w >= old_w) return;
        std::vector<GkVec*> sm = {&U, &Bi}, sn = {&V};
        if (!hlsmr) sn.push_back(&X);                        // (hybrid LSMR re-forms x = V_k y every iteration)
        for (GkVec* s : {&W, &H, &HB, &UN, &XT})
            if (s->p) sn.push_back(s);
        auto move = [&](GkVec* S, GkVec& tmp) {
            for (size_t g = 0; g < ng; ++g) {
                const int nv = (int)std::min<size_t>(SPMM_MAXV, live.size() - g * SPMM_MAXV);
                MvSlots src;
                for (int r = 0; r < SPMM_MAXV; ++r) {
                    src.p[r] = nullptr;
                    src.stride[r] = 1;
                    if (r < nv) {
                        const auto& from = live[g * SPMM_MAXV + r];
                        src.stride[r] = spmm_width((int)groups[from.first].size());
                        src.p[r] = S->at(from.first) + from.second;
                    }
                }
                vk(S->len, nv, 2, [&] { mv_regather(c, S->len, nv, src, tmp.at(g)); });
            }
            std::swap(S->p, tmp.p);
        };
        for (GkVec* s : sm) move(s, tmp_m);
        for (GkVec* s : sn) move(s, tmp_n);
        std::vector<std::vector<int>> next(ng);
        for (size_t i = 0; i < live.size(); ++i) next[i / SPMM_MAXV].push_back(groups[live[i].first][live[i].second]);
        groups.swap(next);
    };

    int running = nrhs;
    for (int k = 0; k < maxit && running > 0; ++k) {
        const bool lastit = k == maxit - 1;
        const bool bstep = !hlsmr || !lastit;                // hybrid lsmr :29: no new v after the last step
        auto for_cols = [&](auto f) {
            for (size_t g = 0; g < groups.size(); ++g)
                for (size_t r = 0; r < groups[g].size(); ++r)
                    if (groups[g][r] >= 0) f(groups[g][r], g, r);
        };
        // ---- u_hat = A*v - alpha*u, beta = norm(u_hat)  (lsqr :22-23, lsmr :34-35, hybrid lsmr :24-25) ----
        for (size_t g = 0; g < groups.size(); ++g) {
            const int nv = (int)groups[g].size();
            const auto& G = groups[g];
            const MvCoef malpha = coef(G, 0.0, [&](int j) { return -alpha[j]; });
            product(A, nv, V.at(g), Tm);
            lin(m, nv, 2, Tm, ones, U.at(g), malpha, nullptr, none, U.at(g), MVS_SQ, nullptr, ds(0, g));
            if (hlsqr)   // lower block of u_hat: (sqrt(lambda)*v) - (alpha*u_n)
                lin(n, nv, 2, V.at(g), coef(G, 0.0, [&](int j) { return sq[j]; }), UN.at(g), malpha, nullptr, none,
                    UN.at(g), MVS_SQ, nullptr, ds(1, g));
        }
        readback(hlsqr ? 2 : 1);
        for_cols([&](int j, size_t g, size_t r) {
            beta[j] = std::sqrt(hlsqr ? hs(0, g, r) + hs(1, g, r) : hs(0, g, r));
            if (hlsmr) {
                Bk[bks * j + (size_t)k * (maxit + 1) + k] = alpha[j];          // :23
                Bk[bks * j + (size_t)k * (maxit + 1) + k + 1] = beta[j];       // :27
            }
        });
        // ---- u = u_hat / beta ; v_hat = A'*u - beta*v, alpha = norm(v_hat)  (lsqr :24-27, lsmr :36-39) ----
        for (size_t g = 0; g < groups.size(); ++g) {
            const int nv = (int)groups[g].size();
            const auto& G = groups[g];
            const MvCoef cbeta = coef(G, 1.0, [&](int j) { return beta[j]; });
            vk(m, nv, 2, [&] { mv_div(c, m, nv, U.at(g), U.at(g), cbeta, plsmr); });
            if (hlsqr) vk(n, nv, 2, [&] { mv_div(c, n, nv, UN.at(g), UN.at(g), cbeta, false); });
            if (!bstep) continue;
            const MvCoef mbeta = coef(G, 0.0, [&](int j) { return -beta[j]; });
            product(At, nv, U.at(g), Tn);
            if (hlsqr)   // (A'*u + sqrt(lambda)*u_n) - beta*v
                lin(n, nv, 3, Tn, ones, UN.at(g), coef(G, 0.0, [&](int j) { return sq[j]; }), V.at(g), mbeta, V.at(g),
                    MVS_SQ, nullptr, ds(0, g));
            else
                lin(n, nv, 2, Tn, ones, V.at(g), mbeta, nullptr, none, V.at(g), MVS_SQ, nullptr, ds(0, g));
        }
        if (bstep) {
            readback(1);
            for_cols([&](int j, size_t g, size_t r) { alpha[j] = std::sqrt(hs(0, g, r)); });
        }
        std::fill(stop.begin(), stop.end(), 0);
        auto hist = [&](double* h, int j) -> double& { return h[(size_t)j * maxit + k]; };
        // b - A*x of one group: ||.||^2 into sums; keep: the residual itself stays in Tm
        auto residual = [&](size_t g, int nv, bool keep, double* sums) {
            product(A, nv, X.at(g), Tm);
            lin(m, nv, 2, Bi.at(g), ones, Tm, minus1, nullptr, none, keep ? Tm : nullptr, MVS_SQ, nullptr, sums);
        };
        if (!lsmr) {
            // ---- LSQR: rotation :31-38, v = v_hat / alpha :28, x and w :40-41, error :43 ----
            for_cols([&](int j, size_t, size_t) {
                lsqr_rotate(beta[j], alpha[j], rho_bar[j], phi_bar[j], c_x[j], c_w[j]);
                if (!hyb) {
                    const double res = std::fabs(phi_bar[j]) / nb[j];          // :44
                    if (res_hist) hist(res_hist, j) = res;
                    stop[j] = res <= tol || lastit;                            // :46 (<=)
                }
            });
            bool any_sum = errmode != MVS_NONE || hyb;
            for (size_t g = 0; g < groups.size(); ++g) {
                const int nv = (int)groups[g].size();
                const auto& G = groups[g];
                vk(n, nv, 6 + (errmode == MVS_DIFF ? 1 : 0), [&] {
                    mv_lsqr_step(c, n, nv, V.at(g), X.at(g), W.at(g), coef(G, 1.0, [&](int j) { return alpha[j]; }),
                                 coef(G, 0.0, [&](int j) { return c_x[j]; }), coef(G, 0.0, [&](int j) { return c_w[j]; }),
                                 errmode, errD(g), ds(0, g));
                });
                // hybrid :43 b - A*x every iteration; lsqr :52 the explicit residual of the columns that stop now
                bool need = hyb;
                for (int j : G) need = need || (j >= 0 && stop[j]);
                if (need) {
                    residual(g, nv, false, ds(1, g));
                    any_sum = true;
                }
            }
            if (any_sum) readback(2);
            for_cols([&](int j, size_t g, size_t r) {
                if (err_hist && xt_in) hist(err_hist, j) = std::sqrt(hs(0, g, r)) / nxt[j];
                if (hyb) {
                    const double res = std::sqrt(hs(1, g, r)) / nb[j];
                    if (res_hist) hist(res_hist, j) = res;
                    stop[j] = res < tol || lastit;                             // hybrid :45 (<)
                } else if (stop[j] && res_hist) {
                    hist(res_hist, j) = std::sqrt(hs(1, g, r)) / nb[j];        // :52
                }
            });
        } else if (plsmr) {
            // ---- LSMR: rotations :42-67, v = v_hat / alpha :40, hbar / x / h :61-67, monitors :69-73 ----
            for_cols([&](int j, size_t, size_t) {
                double cfm[5], cfn[5];
                lsmr_rotate(beta[j], alpha[j], &rot[(size_t)9 * j], &cf[(size_t)3 * j], cfm, cfn);
            });
            for (size_t g = 0; g < groups.size(); ++g) {
                const int nv = (int)groups[g].size();
                const auto& G = groups[g];
                vk(n, nv, 8 + (errmode == MVS_DIFF ? 1 : 0), [&] {
                    mv_lsmr_step(c, n, nv, V.at(g), X.at(g), H.at(g), HB.at(g),
                                 coef(G, 1.0, [&](int j) { return alpha[j]; }),
                                 coef(G, 0.0, [&](int j) { return cf[(size_t)3 * j]; }),
                                 coef(G, 0.0, [&](int j) { return cf[(size_t)3 * j + 1]; }),
                                 coef(G, 0.0, [&](int j) { return cf[(size_t)3 * j + 2]; }), k == 0, errmode, errD(g),
                                 ds(0, g));
                });
                residual(g, nv, true, ds(1, g));                               // :69 r = b - A*x
                product(At, nv, Tm, Tn);                                       // :71 A.'*r
                lin(n, nv, 1, Tn, ones, nullptr, none, nullptr, none, nullptr, MVS_SQ, nullptr, ds(2, g));
            }
            readback(3);
            for_cols([&](int j, size_t g, size_t r) {
                const double nr = std::sqrt(hs(1, g, r));
                const double res = nr / (nb[j] + EPSD);                        // :70
                if (res_hist) hist(res_hist, j) = res;
                if (ar_hist) hist(ar_hist, j) = std::sqrt(hs(2, g, r)) / (normA * std::max(nr, EPSD));   // :71
                if (err_hist && xt_in) hist(err_hist, j) = std::sqrt(hs(0, g, r)) / nxt[j];              // :72-73
                stop[j] = res < tol || lastit;                                 // :76 (<)
            });
        } else {
            // ---- hybrid LSMR: V(:,k+1) :32-33, the projected solve :37-44, x = V_k y :45, monitors :47-48 ----
            const int kk = k + 1;
            for (size_t g = 0; g < groups.size() && bstep; ++g) {
                const int nv = (int)groups[g].size();
                const auto& G = groups[g];
                vk(n, nv, 2, [&] { mv_div(c, n, nv, V.at(g), V.at(g), coef(G, 1.0, [&](int j) { return alpha[j]; }), false); });
                vk(n, nv, 2, [&] {
                    mv_unpack(c, n, nv, V.at(g), ptrs(G, [&](int j) { return Vj(j) + (size_t)kk * ldn; }, dump));
                });
            }
            // (without a new v, :34 keeps the previous alpha: alpha[j] is untouched when !bstep)
            for_cols([&](int j, size_t, size_t) {
                dense::proj_hybrid_lsmr(&Bk[bks * j], maxit + 1, kk, alpha[j], beta[j], beta1[j], lambdas[j],
                                        &Yh[(size_t)maxit * j]);
            });
            h2d(c, Yd, Yh.data(), sizeof(double) * Yh.size());
            for_cols([&](int j, size_t, size_t) {
                gemv<double>(c, n, kk, Vj(j), ldn, Yd + (size_t)maxit * j, xj(j), 0);                     // :45
            });
            for (size_t g = 0; g < groups.size(); ++g) {
                const int nv = (int)groups[g].size();
                const auto& G = groups[g];
                vk(n, nv, 2, [&] { mv_pack(c, n, nv, ptrs(G, xj, dump), X.at(g)); });
                if (errmode != MVS_NONE)                                       // :47
                    lin(n, nv, 1, X.at(g), ones, nullptr, none, nullptr, none, nullptr, errmode, errD(g), ds(0, g));
                residual(g, nv, false, ds(1, g));                              // :48
            }
            readback(2);
            for_cols([&](int j, size_t g, size_t r) {
                const double res = std::sqrt(hs(1, g, r)) / nb[j];
                if (res_hist) hist(res_hist, j) = res;
                if (err_hist && xt_in) hist(err_hist, j) = std::sqrt(hs(0, g, r)) / nxt[j];
                stop[j] = res <= tol || lastit;                                // :50 (<=)
            });
        }
        // ---- the columns that stop leave the batch with their x ----
        bool left = false;
        for (size_t g = 0; g < groups.size(); ++g) {
            auto& G = groups[g];
            bool here = false;
            for (int j : G) here = here || (j >= 0 && stop[j]);
            if (!here) continue;
            left = true;
            const int nv = (int)G.size();
            if (!hlsmr) vk(n, nv, 2, [&] { mv_unpack(c, n, nv, X.at(g), ptrs(G, xj, dump)); });
            for (int& j : G)
                if (j >= 0 && stop[j]) {
                    niters[j] = k + 1;
                    --running;
                    j = -1;
                }
        }
        if (left && running > 0) regather();
    }
    cb.stage_out(c, X_out, ldx);
    return HGM_OK;
}

// explicit instantiations used by capi.cpp
template int lsqr_t<double>(hgm_ctx*, const hgm_opts*, const hgm_mat*, const hgm_mat*, const double*, const double*,
                            double, int, bool, double, double*, double*, double*, int*);
template int lsqr_t<float>(hgm_ctx*, const hgm_opts*, const hgm_mat*, const hgm_mat*, const double*, const double*,
                           double, int, bool, double, double*, double*, double*, int*);
template int lsmr_t<double>(hgm_ctx*, const hgm_opts*, const hgm_mat*, const hgm_mat*, const double*, const double*,
                            double, int, double*, double*, double*, double*, int*);
template int lsmr_t<float>(hgm_ctx*, const hgm_opts*, const hgm_mat*, const hgm_mat*, const double*, const double*,
                           double, int, double*, double*, double*, double*, int*);

}  // namespace hgm
