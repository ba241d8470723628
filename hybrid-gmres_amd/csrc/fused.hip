// One pass over B for the m-space Arnoldi operator w = A*(B*q) (ABgmres_*_bounds.m:25,
// gcv_function.m:20) when B is A' value for value (a device transpose pair) -- DESIGN.md §3.5.
//
// The two-pass form streams the same values twice (B*q pixel-major, then A*z ray-major: 24.5 GB
// of algorithmic traffic per step at C4).  Here B's pixel-major entries are read ONCE:
//   z_j = sum_i B(j,i) q_i                  (row sums: the kept column B*q, written out)
//   w_i = sum_j A(i,j) z_j = sum_j B(j,i) z_j
// The second sum scatters from pixel rows into rays.  To keep it deterministic (no atomics) and
// its partials few, the pixels are grouped into REGIONS (R x R pixel squares of the image): one
// workgroup owns one region and accumulates the region's rays in LDS (a 64 x 64 square is
// crossed by ~3,900 of the 272,271 C4 rays), so one partial per (region, ray) leaves the kernel;
// a ray-major pass then sums each ray's partials in region order.
//
// The pixel rows of a region are shared out among the workgroup's waves; each wave walks its rows
// in a fixed order and adds into accumulators of its own, so every sum has a fixed order and the
// products are bitwise reproducible ("Row-wave pass" below).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <numeric>
#include <thread>

#include "device_common.h"

namespace hgm {

// The shape of the row-wave pass (k_fused_rw): waves per region and pixel rows per load batch.
// Other shapes were measured and retired.
constexpr int RW_WAVES = 4;
constexpr int RW_ROWS = 8;

struct FusedPlan {
    int elem = 8;                 // value size (fp64 or fp32; the slots are byte offsets)
    int region = 0, maxr = 0;     // pixel square per workgroup; LDS ray slots (RwSlots)
    bool rowpair = false;         // units of two consecutive rows (k_fused_rw PAIRS; runs split so
                                  // every unit spans one chunk)
    int64_t nreg = 0, nslot = 0, m = 0, maxlen = 0;
    // per (region, wave) a range of row runs; the region's rays; every entry's index among its
    // region's rays
    int32_t* wrun = nullptr;      // nreg * RW_WAVES + 1
    int2* runs = nullptr;         // (first row, rows)
    int32_t* ray_tab = nullptr;   // nslot: global ray of each region-local ray
    uint16_t* lidx = nullptr;     // nnz (+ padding): the slot as an LDS byte offset (index * elem)
    int64_t* reg_base = nullptr;  // nreg+1
    int64_t* rs_ptr = nullptr;    // m+1
    int32_t* rs_slot = nullptr;   // nslot
    // the partials by ray band (k_fused_reduce_band): band b = rays [64 b, 64 b + 64); its
    // runs (first slot, first ray - 64 b, rays) of consecutive rays in consecutive slots of one
    // region, regions in increasing order
    int64_t nband = 0, nrun = 0;
    int32_t* band_ptr = nullptr;  // nband + 1
    int4* band_run = nullptr;     // nrun
    double* part = nullptr;       // nslot (fp32 plans use it as float)
    double* zx_part = nullptr;    // nreg (the regions' side sums; fp32 plans: float)
    double build_s = 0;
    bool dev_built = false;       // ray sets built on the device (HGM_OPT_FUSED_PLAN_DEV)
    // fp64 row pairs: the compact value stream (HGM_OPT_FUSED_VSTREAM, k_fused_rw COMPACT;
    // "Compact value stream" below).  lidx stays: the Golub-Kahan form of the pass reads the plain streams.
    bool vs_on = false;           // the pass reads the compact streams
    int64_t nunit = 0, vs_pairs = 0, vs_coded = 0;   // units, 16-byte value pairs, entries with a code
    int64_t nnz = 0, nwrun = 0;                      // B's entries, the row runs of `runs`
    uint2* vs_desc = nullptr;     // nunit + 1: (first value pair, first-row entries | first-row coded pairs << 8)
    int32_t* vs_run_unit = nullptr;   // per run of `runs`: its first unit
    double* vs_table = nullptr;   // 32: entry 31 - c = the value of code c (code 0: -0.0)
    uint32_t* vs_slots = nullptr; // 64 words per unit: lane l's two slots and codes
    double* vs_vals = nullptr;    // 2 * vs_pairs
};

void fused_plan_free(FusedPlan* P) {
    if (!P) return;
    for (void* p : {(void*)P->reg_base, (void*)P->rs_ptr, (void*)P->rs_slot, (void*)P->part, (void*)P->wrun,
                    (void*)P->runs, (void*)P->ray_tab, (void*)P->lidx, (void*)P->zx_part, (void*)P->band_ptr,
                    (void*)P->band_run, (void*)P->vs_desc, (void*)P->vs_run_unit, (void*)P->vs_table,
                    (void*)P->vs_slots, (void*)P->vs_vals})
        if (p) (void)hipFree(p);
    delete P;
}

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
// w_i = sum of ray i's region partials.  RG lanes per ray: lane l takes the ray's partials l, l+RG,
// ... in region order, then the RG lane sums are added by a fixed tree: the slot indices of a ray are
// read contiguously across its lanes.  (Fewer lanes per ray measured slower: DESIGN.md §3.5.)
// With zx_out, block 0 first adds the nzx regional shares of the side dot x_true'(B*q) (fixed
// order) into *zx_out.
constexpr int RG = 8;
using ReduceBatches = Ints<4, 8, 16>;            // RB: partials per lane in flight (fused_pass picks by ppl)
template <typename T, int RB>
__global__ __launch_bounds__(BS) void k_fused_reduce(int64_t m, const int64_t* __restrict__ rs_ptr,
                                                     const int32_t* __restrict__ rs_slot,
                                                     const T* __restrict__ part, T* __restrict__ w,
                                                     const T* __restrict__ zx_part, int nzx, T* zx_out) {
    if (zx_out && blockIdx.x == 0) {
        __shared__ T sh[4];
        const T t = reduce_parts<T, false>(zx_part, nzx, sh);
        if (threadIdx.x == 0) st_sys(zx_out, t);           // (the host ring: system scope, device_common.h)
    }
    const int gl = threadIdx.x % RG;
    for (int64_t i = ((int64_t)blockIdx.x * BS + threadIdx.x) / RG; i < m; i += (int64_t)gridDim.x * (BS / RG)) {
        T s = T(0);
        const int64_t k0 = rs_ptr[i], k1 = rs_ptr[i + 1];
        int64_t k = k0 + gl;
        // a ray's partials in batches of RB per lane with the batch's tail clamped to the ray's
        // last slot (read again, not added): every slot read, then every partial read in flight
        // (C4: ~14 partials per lane, one batch instead of three batches and a serial tail).  The
        // lane adds its partials in slot order whatever RB is, so every RB gives the same bits;
        // the host sizes RB to the partials per lane (fused_pass: a pixel shard's rays
        // cross few of its regions)
        for (; k < k1; k += RB * RG) {
            int32_t sl[RB];
            T p[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) sl[u] = rs_slot[std::min<int64_t>(k + u * RG, k1 - 1)];
#pragma unroll
            for (int u = 0; u < RB; ++u) p[u] = part[sl[u]];
#pragma unroll
            for (int u = 0; u < RB; ++u)
                if (k + u * RG < k1) s += p[u];
        }
        // (the batches above leave nothing for these two loops; the compiler keeps them for RB 4, and
        // they stay so that every instance compiles to the instructions it had)
        for (; RB < 8 && k + (RB - 1) * RG < k1; k += RB * RG) {   // RB slot reads, then RB partial reads in flight
            int32_t sl[RB];
            T p[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) sl[u] = rs_slot[k + u * RG];
#pragma unroll
            for (int u = 0; u < RB; ++u) p[u] = part[sl[u]];
#pragma unroll
            for (int u = 0; u < RB; ++u) s += p[u];
        }
        for (; k < k1; k += RG) s += part[rs_slot[k]];
        s = group_sum<T, RG>(s);
        if (gl == 0) w[i] = s;
    }
}

// The same sums by ray band (HGM_OPT_FUSED_REDUCE = 1; measured 2-4 % slower, off by default): one wave per
// band of 64 consecutive rays, lane l owning ray 64 b + l.  The band's runs come in region order;
// a lane adds each partial of its ray to accumulator (j mod 8), j = the partial's index in the
// ray's region-ordered list -- the exact sums lane j mod 8 of k_fused_reduce forms -- and the 8
// accumulators of a ray then go through the same group_sum<8>: the bits of k_fused_reduce.  The
// partials are read in runs of consecutive slots (coalesced) instead of through the 4-B rs_slot
// gather (C4: 126 MB less per pass).  RUNB runs' loads are issued before their adds.
constexpr int RUNB = 16;
template <typename T>
__global__ __launch_bounds__(BS) void k_fused_reduce_band(int64_t m, int64_t nband, const int32_t* __restrict__ band_ptr,
                                                          const int4* __restrict__ band_run,
                                                          const T* __restrict__ part, T* __restrict__ w,
                                                          const T* __restrict__ zx_part, int nzx, T* zx_out) {
    __shared__ T tr[BS / 64][64][9];             // per wave: the lanes' 8 sums (+1: bank spread)
    if (zx_out && blockIdx.x == 0) {
        __shared__ T sh[4];
        const T t = reduce_parts<T, false>(zx_part, nzx, sh);
        if (threadIdx.x == 0) st_sys(zx_out, t);
    }
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int64_t band = (int64_t)blockIdx.x * (BS / 64) + wv;
    if (band >= nband) return;                    // (a whole wave: no barrier follows)
    T a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, a5 = 0, a6 = 0, a7 = 0;
    int jc = 0;
    const int r0 = band_ptr[band], r1 = band_ptr[band + 1];
    for (int rc = r0; rc < r1; rc += 64) {
        const int nr = min(64, r1 - rc);
        const int4 d = ln < nr ? band_run[rc + ln] : make_int4(0, 0, 0, 0);
        for (int rb = 0; rb < nr; rb += RUNB) {
            T p[RUNB];
            bool in[RUNB];
#pragma unroll
            for (int u = 0; u < RUNB; ++u) {      // the loads of RUNB runs first (runs past nr: empty)
                const int r = min(rb + u, 63);
                const int slo = __builtin_amdgcn_readlane(d.x, r), rlo = __builtin_amdgcn_readlane(d.y, r);
                const int cnt = rb + u < nr ? __builtin_amdgcn_readlane(d.z, r) : 0;
                in[u] = (unsigned)(ln - rlo) < (unsigned)cnt;
                p[u] = part[in[u] ? slo + (ln - rlo) : slo];
            }
#pragma unroll
            for (int u = 0; u < RUNB; ++u) {      // then the adds, in run (= region) order
                const int g = jc & 7;
                a0 = (in[u] && g == 0) ? a0 + p[u] : a0;
                a1 = (in[u] && g == 1) ? a1 + p[u] : a1;
                a2 = (in[u] && g == 2) ? a2 + p[u] : a2;
                a3 = (in[u] && g == 3) ? a3 + p[u] : a3;
                a4 = (in[u] && g == 4) ? a4 + p[u] : a4;
                a5 = (in[u] && g == 5) ? a5 + p[u] : a5;
                a6 = (in[u] && g == 6) ? a6 + p[u] : a6;
                a7 = (in[u] && g == 7) ? a7 + p[u] : a7;
                jc += in[u] ? 1 : 0;
            }
        }
    }
    T* t = tr[wv][ln];
    t[0] = a0; t[1] = a1; t[2] = a2; t[3] = a3; t[4] = a4; t[5] = a5; t[6] = a6; t[7] = a7;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (one wave: its LDS accesses run in order)
    const int64_t ray0 = band * 64;
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {              // 8 rays at a time: lanes 8i..8i+7 = ray 8 s8 + i
        const int rr = s8 * 8 + (ln >> 3);
        T v = tr[wv][rr][ln & 7];
        v = group_sum<T, 8>(v);
        if ((ln & 7) == 0 && ray0 + rr < m) w[ray0 + rr] = v;
    }
}

// ------------------------------------------------------------------------------------------
// Row-wave pass.  One workgroup of W waves per region; the region's rays get LDS
// slots: q of each ray (shared) and one accumulator per wave (private).  A wave walks its share
// of the region's pixel rows one row at a time, the row's entries across its 64 lanes, two per
// lane (NCH chunks of 128): p = v * q[slot] in registers, z_j = the wave sum of p (fixed tree), then
// acc[slot] += v * z_j.  A pixel row meets each ray at most once, so the lanes of one row hit
// distinct slots: no conflicts, no atomics, no barriers; the wave's rows go in a fixed order and
// the W accumulators are added in wave order at the end, so every sum has a fixed order.
// Per entry the pass reads the value (8 B) and its slot (2 B) once, and touches the LDS three
// times (q read, accumulator read and write).
//
// Loads are software-pipelined in batches of G rows (never crossing a run of consecutive rows):
// the row pointers of batch b+2 and the entries of batch b+1 are in flight while batch b is
// processed.  Every load goes through a buffer resource sized to its row (past the end: 0), so
// each batch issues the same instructions and the compiler's in-order vmcnt waits stay exact.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t readlane64(int64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Lane exchanges of gfx950 for a transposed reduction (fp64 as two dwords): swap32 swaps lanes
// 32-63 of a with lanes 0-31 of b, swap16 the odd 16-lane rows of a with the even rows of b.
__device__ __forceinline__ void swap32(double& a, double& b) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap16(double& a, double& b) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void swap32(float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    a = __uint_as_float(r[0]);
    b = __uint_as_float(r[1]);
}
// The 64-lane sums of G values at once (G = 4 or 8), by a butterfly that halves the values per
// lane while it halves the lanes per sum: lane l ends with the sum of P[l / (64 / G)], the same
// bits in each lane of its group.  Fixed order.  Per row this is ~6 exchanges and adds instead of
// a full wave reduction each (DPP tree + 8 readlanes).
template <int G, typename T>
__device__ __forceinline__ T rows_sum_t(T (&P)[G]) {
    static_assert(G == 4 || G == 8, "rows per batch");
#pragma unroll
    for (int i = 0; i < G / 2; ++i) {          // lane bit 5
        swap32(P[i], P[i + G / 2]);
        P[i] = P[i] + P[i + G / 2];
    }
#pragma unroll
    for (int i = 0; i < G / 4; ++i) {          // lane bit 4
        swap16(P[i], P[i + G / 4]);
        P[i] = P[i] + P[i + G / 4];
    }
    if constexpr (G == 8) {                    // lane bit 3: row_ror 8 within 16-lane rows
        const bool hi = (threadIdx.x & 8) != 0;
        T s = hi ? P[1] : P[0];
        const T t = hi ? P[0] : P[1];
        s = s + dpp_mov<0x128>(t);
        s += dpp_mov<0xB1>(s);                 // lane ^ 1
        s += dpp_mov<0x4E>(s);                 // lane ^ 2
        s += dpp_mov<0x141>(s);                // other quad of the 8-lane half
        return s;
    } else {
        return row16_sum(P[0]);
    }
}

// acc += t in the LDS unit (ds_add_f64, no return value): the update needs no round trip.
// DETERMINISM INVARIANT: the order of the adds into one accumulator is
// fixed because (1) the accumulator array is private to the wave (acc[wv]), (2) the LDS executes
// one wave's DS instructions in issue order, and (3) within one instruction the 64 lanes address
// distinct slots (a pixel row meets a ray at most once; out-of-row lanes use their own dummy slot).
// So no atomicity is involved -- only an in-place read-modify-write in program order -- and the
// sums are bitwise reproducible (test_gpu_fused.py repeats every product and solve bit for bit).
// Breaking any of (1)-(3) (shared accumulators, a second wave, duplicate slots per row) would
// make the order depend on timing.
template <typename T>
__device__ __forceinline__ void lds_add(T* p, T t) {
    (void)__hip_atomic_fetch_add(p, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// The products of the paired forms and the fp32 accumulator updates are fused multiply-adds (one
// rounding per term instead of two: half the VALU; the library otherwise builds with
// -ffp-contract=off for MATLAB's epilogues).
__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }
// cache policy of the pass's entry stream (values, slots): the default (0); nt (2) measured
// 1.7-2.2 % slower (a unit's chunk shares its boundary lines with the next unit's)
constexpr int RW_AUX = 0;

// The forms of the pass (the retired ones and their measurements: DESIGN.md §3.5).  A batch is
// RW_ROWS rows; a lane holds two entries of a chunk of 128 (a 16-byte value pair (8-byte in fp32)
// and a 4-byte slot pair from the row's pair-aligned start).
//   ROWS     one row per chunk, NCH chunks per row.
//   PAIRS    the rows of a batch go as units of two consecutive rows, whose entries are contiguous
//            in B's CSR: one chunk from the unit's first pair carries both rows (the first row
//            from lane 0, the second right after it), so a row of ~60 entries no longer leaves
//            half the lanes idle.  q is read through two addresses per entry, the entry's slot
//            for its own row and the lane's dummy slot (q = 0) for the other, which splits the
//            products by row into P[2u] / P[2u+1] without selects (the butterfly then sums rows
//            exactly as in ROWS); each unit's two rows are added by two instructions, every
//            lane of the other row on its dummy slot.  The plan keeps every unit's span within
//            one chunk (fused_plan_build_rw splits runs).
//   COMPACT  (compact value stream, HGM_OPT_FUSED_VSTREAM; fp64, GK = false) is PAIRS reading
//            plan-owned streams instead of B's values, the plan's lidx and B's row pointers; below.
// COMPACT: the up to 31 most frequent value bit patterns of the operator are CODES; only the other
// values (ESCAPES) are stored.  A unit's entries are reordered at plan time into
//     [first row coded | first row escapes | second row escapes | second row coded]  (<= 128),
// so an entry belongs to the first row iff its position is below the first row's length (one
// compare, no unit offset), and the escapes are one contiguous stretch:
//   slots   64 words per unit, lane l's word = positions 2l, 2l+1: slot offsets in bits 3-13 and 19-29,
//           the code of 2l in bits 14-18, of 2l+1 in bits 30-31 (low) and 0-2 (high); positions past
//           the unit carry their lane's dummy slot and code 0, so the kernel needs no "inside" test;
//   values  the escapes as 16-byte pairs: pair j = positions 2 (c0h + j), +1 with c0h = (first row's
//           coded) / 2; a position that is not an escape holds 0.0;
//   descriptor (8 B per unit, instead of the row pointers): first value pair, first row's entries,
//           c0h; the next unit's first pair ends this one's.
// Decode without a select: v = loaded + table[code] with table[0] = -0.0 (x + -0.0 = x for every x,
// -0.0 included) and loaded = 0.0 wherever the entry is coded (0.0 + t = t for the finite non-zero
// t the dictionary holds): bit for bit the stored value.  The table sits in the q slots below the
// dummies, code c at slot MAXR - 65 - c (the word's 5-bit field holds 31 - c, so the offset is an
// immediate plus field * 8); the plan keeps as many codes as the fullest region leaves slots for
// (rays <= MAXR - 65 - codes; C4: 1,924 rays in 1,984 ray slots, all 31 codes).
enum Form { ROWS, PAIRS, COMPACT };
struct VStream {
    const uint2* desc = nullptr;
    const int32_t* run_unit = nullptr;
    const double* table = nullptr;
};
// The instantiated shapes, from which the plan and the launch both choose: LDS ray slots (64 of
// them the lanes' dummies; the plan takes the fewest that hold its regions' rays: more workgroups
// per CU), chunks per row of ROWS, load-ring depths of COMPACT (depth 4 measured no faster).
// The slots are listed once, as (waves, slots) pairs in the form tests/fused_cases.py has always read
// from this file (the twin of the plan rules takes its shapes from here); RwSlots is that list.
#ifdef HGM_RW_SHAPES
#error "HGM_RW_SHAPES is this file's list of LDS shapes"
#else
#define HGM_RW_SHAPES(X) X(4, 1088) X(4, 1344) X(4, 1536) X(4, 2048)
#endif
#define HGM_RW_SHAPE_SLOTS(WV, MRV) , MRV
#define HGM_RW_SHAPE_WAVES(WV, MRV) && WV == RW_WAVES
template <int, int... Vs>
struct IntsAfterFirst { using type = Ints<Vs...>; };
using RwSlots = IntsAfterFirst<0 HGM_RW_SHAPES(HGM_RW_SHAPE_SLOTS)>::type;
static_assert(true HGM_RW_SHAPES(HGM_RW_SHAPE_WAVES), "every shape has RW_WAVES waves");
#undef HGM_RW_SHAPE_SLOTS
#undef HGM_RW_SHAPE_WAVES
using RwChunks = Ints<1, 2>;
using RwCompactDepths = Ints<2, 3>;
constexpr int RW_DEPTH = 2;                      // the load ring of ROWS and PAIRS

// T: double (the GMRES family) or float (BASELINE configs[4], the Golub-Kahan path in fp32): the
// values, q, the row sums, the LDS slots and the partials are T; slots are LDS byte offsets
// (slot * sizeof(T), the plan's element size).  The accumulators are updated by lds_add in fp64 and
// by read-add-write (ds_read_b32, v_add_f32, ds_write_b32; a wave's rows in order) in fp32: the
// no-return fp32 LDS add runs at a fraction of ds_add_f64's rate on gfx950 (11.3 ms against
// 2.00 ms at C5; profiles/r4_micro_f32.jsonl).
// D: batches in the ring (D - 1 in flight while one is processed).
//
// Row epilogue (the Golub-Kahan step v_hat = A'*u - beta*v of lsqr_solver.m:26 / lsmr_solver.m:38
// with q = u): zs_j = z_j - a * ev[j] with a = (T)sqrt((double)*easq), two roundings (no FMA, as
// the two-pass EPI_SUB epilogue); the scatter then forms A*zs, i.e. A*v_hat, so the next step's
// A*v_{k+1} = (A*v_hat)/alpha needs no second pass over the operator.  Without ev: zs = z - 0*0,
// the same bits as z.  Outputs (either may be null): zraw[j] = z_j, zout[j] = zs_j (zout may be ev:
// a row is read and written by the same lanes of one wave, read first).
// Side sum (one value per region, in zx_part): side_sq == 0: sum_j zs_j * xt[j] (the m-space Gram
// error monitor's x_true'(B*q)); side_sq == 1: sum_j zs_j^2 (alpha^2 of the Golub-Kahan step).
// GK: the row epilogue / zout / side_sq code exists (false: the GMRES family's instruction stream).
// pn (pending normalisation of q, the m-space AB-GMRES step; internal.h PendNorm, pn.np > 0): q still
// holds the previous MGS sweep's unnormalised v; every wave re-reduces the sweep's norm partials
// exactly as k_mgs_normalize does (stride BS, then block_sum_all: the same bits), h = sqrt(sum), and
// stages q = v / h (v when h = 0, as k_mgs_normalize leaves it) into its LDS slots; workgroup 0
// publishes h to pn.hdev and H(k+1,k) of the host ring (the MGS sweep that follows writes q back).
template <typename T, bool GK, int MAXR, int NCH, int D, Form F>
__global__ __launch_bounds__(64 * RW_WAVES) void k_fused_rw(const int64_t* __restrict__ reg_base, const int32_t* __restrict__ ray_tab,
                                                            const int32_t* __restrict__ wrun, const int2* __restrict__ runs,
                                                            const int64_t* __restrict__ rp, const T* __restrict__ val,
                                                            const uint16_t* __restrict__ lidx, const T* __restrict__ q,
                                                            T* __restrict__ zraw, T* __restrict__ part,
                                                            const T* __restrict__ xt, T* __restrict__ zx_part,
                                                            const T* ev, const T* __restrict__ easq, T* zout, int side_sq,
                                                            PendNorm<T> pn, VStream vs) {
    constexpr int W = RW_WAVES, G = RW_ROWS;
    static_assert(D >= 2 && D <= 4, "ring depth");
    static_assert(F == ROWS || NCH == 1, "row pairs: one chunk");
    constexpr bool VS = F == COMPACT;            // compact value stream: val = the escapes, lidx = the unit words
    static_assert(!VS || (sizeof(T) == 8 && !GK && MAXR <= 2048), "compact value stream: fp64 GMRES form");
    constexpr int VTAB = MAXR - 96;              // (VS) the code table's first q slot
    constexpr int EPL = 2;                       // entries per lane per chunk
    constexpr int CH = 64 * EPL;                 // entries per chunk
    constexpr int ES = (int)sizeof(T);
    constexpr bool RAW = ES == 4;                // accumulators by read-add-write (fp32), else lds_add
    // One shared object, q first: two __shared__ arrays are laid out by size, the accumulators
    // at offset 0 and q behind them, past the 16-bit offset field of the DS instructions, and
    // every q, table and dummy access then pays a VALU add of q's base.  With q at 0 those are
    // immediates on the slot registers.
    struct Lds {
        T q[MAXR];                               // (the last 64: the lanes' dummy slots)
        T acc[W][MAXR];
    };
    __shared__ Lds lds;
    T(&qloc)[MAXR] = lds.q;
    T(&acc)[W][MAXR] = lds.acc;
    const int g = blockIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ln = threadIdx.x & 63;
    const int64_t pb = reg_base[g];
    const int nr = (int)(reg_base[g + 1] - pb);
    // Staging: q at the region's rays into LDS, the accumulators zeroed.  All ray_tab loads, then all
    // q gathers, are issued before any is used (NQ per thread), so the pending-normalisation sum
    // below overlaps them.
    // Pending normalisation (pn.np > 0): h = sqrt(sum of pn.parts) in reduce_parts' order for a
    // BS-thread block (thread t sums parts t, t + BS, ...; wave sums; (s0 + s1) + (s2 + s3)), which
    // every wave forms by itself for the BS / 64 virtual waves: the bits of k_mgs_normalize's h with
    // no barrier and no LDS.
    // the wave's runs (<= 64, the plan checks) in lanes: readlane in the loop, no loads there (a
    // conditional load makes the compiler wait for every load in flight after it, and scalar loads'
    // lgkmcnt waits would also wait on the LDS); a range-checked buffer load (zeros past the wave's
    // runs) issued before the staging, so it is in flight with it (round 6)
    int ua = wrun[g * W + wv];
    const int ub = wrun[g * W + wv + 1];
    const int2 runv = __builtin_bit_cast(
        int2, __builtin_amdgcn_raw_buffer_load_b64(buf_rsrc(runs + ua, (ub - ua) * 8), ln * 8, 0, 0));
    int runu = 0;                                // (VS) the first unit of each of the wave's runs
    T tabv = T(0);                               // (VS) the code table, entry threadIdx.x of 32
    if constexpr (VS) {
        runu = (int)__builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(vs.run_unit + ua, (ub - ua) * 4), ln * 4, 0, 0);
        tabv = (T)vs.table[threadIdx.x & 31];
    }
    static_assert(BS == 256 && MAX_PARTS <= 4 * BS, "pending-normalisation sum: four virtual waves");
    T hq = T(0);
    auto pend_h = [&]() -> T {
        // range-checked buffer loads (zeros past np; adding +0 to a sum of squares changes no bit),
        // all 16 in flight before the sums
        const __amdgpu_buffer_rsrc_t rpp = buf_rsrc(pn.parts, pn.np * (int)sizeof(T));
        T pv[4][4];
#pragma unroll
        for (int vw = 0; vw < 4; ++vw)
#pragma unroll
            for (int j = 0; j < 4; ++j) pv[vw][j] = buf_load<T>(rpp, (64 * vw + ln + j * BS) * (int)sizeof(T));
        T s[4];
#pragma unroll
        for (int vw = 0; vw < 4; ++vw) {
            T a = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) a += pv[vw][j];
            s[vw] = wave_sum(a);
        }
        const T h = sqrt((s[0] + s[1]) + (s[2] + s[3]));
        if (g == 0 && threadIdx.x == 0) {
            pn.hdev[0] = h;
            st_sys(pn.hring, h);
        }
        return h;
    };
    constexpr int NQ = (MAXR - 64 + 64 * W - 1) / (64 * W);   // staging iterations per thread
    static_assert(NQ <= 8, "the staging loads go out at once (registers)");
    // branch-free: a range-checked buffer load returns ray 0 past nr (q[0] is read, not stored), so
    // the NQ ray_tab loads and then the NQ gathers each go out with one wait; their stores into the
    // LDS come after the first batches' row pointers are issued (below), so those are in flight
    // with the gathers (round 6)
    T qv[NQ];
    const __amdgpu_buffer_rsrc_t rrt = buf_rsrc(ray_tab + pb, nr * 4);
    int rt[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u)
        rt[u] = (int)__builtin_amdgcn_raw_buffer_load_b32(rrt, (int)(threadIdx.x + u * 64 * W) * 4, 0, 0);
#pragma unroll
    for (int u = 0; u < NQ; ++u) qv[u] = q[rt[u]];
    auto stage = [&]() {
        if (pn.np > 0) hq = pend_h();
        if (hq != T(0)) {                    // (uniform: no divisions without the pending norm)
#pragma unroll
            for (int u = 0; u < NQ; ++u) qv[u] = qv[u] / hq;
        }
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
            const int k = threadIdx.x + u * 64 * W;
            if (k < nr) {
                qloc[k] = qv[u];
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w][k] = T(0);
            }
        }
        if (threadIdx.x < 64) qloc[MAXR - 64 + threadIdx.x] = T(0);
        if constexpr (VS) {
            // (entries below the plan's codes are unused: those slots may hold rays)
            if (threadIdx.x < 32 && VTAB + (int)threadIdx.x >= nr) qloc[VTAB + threadIdx.x] = tabv;
        }
    };
    // the epilogue coefficient: the bits the host takes from the same sum of squares
    const T ea = (GK && easq) ? (T)sqrt((double)*easq) : T(0);
    // (the barrier that publishes the staging sits after the first batches' loads are issued, below:
    // their row pointers and entries are in flight with the staging; round 6)
    T* __restrict__ ac = &acc[wv][0];
    int u = ua, o = 0;
    auto next = [&](int& r0, int& cnt, int& un) {
        r0 = 0;
        cnt = 0;
        un = 0;
        if (u >= ub) return;
        const int rr = __builtin_amdgcn_readlane(runv.x, u - ua), rn = __builtin_amdgcn_readlane(runv.y, u - ua);
        if constexpr (VS) un = __builtin_amdgcn_readlane(runu, u - ua) + (o >> 1);   // (batches start at even rows)
        r0 = rr + o;
        cnt = min(G, rn - o);
        o += cnt;
        if (o == rn) {
            ++u;
            o = 0;
        }
    };
    // row pointers of a batch: lane j holds rp[r0 + min(j, cnt)] (rows past cnt are empty)
    auto load_rp = [&](int r0, int cnt, int un) -> int64_t {
        if constexpr (VS) {
            // the unit descriptors instead: lane j holds unit un + min(j, units) (the last: the batch's end)
            const int nu = (cnt + 1) >> 1;
            const __amdgpu_buffer_rsrc_t r = buf_rsrc(vs.desc + un, (nu + 1) * 8);
            return __builtin_bit_cast(int64_t, __builtin_amdgcn_raw_buffer_load_b64(r, min(ln, nu) * 8, 0, 0));
        }
        const __amdgpu_buffer_rsrc_t r = buf_rsrc(rp + r0, (cnt + 1) * 8);
        return __builtin_bit_cast(int64_t, __builtin_amdgcn_raw_buffer_load_b64(r, min(ln, cnt) * 8, 0, 0));
    };
    constexpr int GL = 64 / G;                    // lanes per row sum after the butterfly
    struct RB {
        int r0, cnt;
        int len[G], off[G];
        T v[G][NCH][EPL];
        uint32_t s[G][NCH];
        T xv;                                     // x_true of row l / GL at lane l (side dot)
        T evv;                                    // ev of row l / GL at lane l (row epilogue)
    };
    // lane l / GL's row of the batch at the group's first lane, past every range elsewhere
    auto row_off = [&]() { return (ln & (GL - 1)) == 0 ? (ln / GL) * ES : (1 << 30); };
    auto issue = [&](RB& b, int r0, int cnt, int64_t rpv, int un) {
        b.r0 = r0;
        b.cnt = cnt;
        (void)un;
        {   // (no xt / ev: an empty range, no memory access)
            const __amdgpu_buffer_rsrc_t rx = buf_rsrc(xt + r0, xt ? cnt * ES : 0);
            b.xv = buf_load<T>(rx, row_off());
            if constexpr (GK) {
                const __amdgpu_buffer_rsrc_t re = buf_rsrc(ev + r0, ev ? cnt * ES : 0);
                b.evv = buf_load<T>(re, row_off());
            } else {
                b.evv = T(0);
            }
        }
        if constexpr (VS) {
            // the batch's units are consecutive in both streams: one resource each, a unit is an SGPR
            // offset into it; b.len[2u] = the first row's entries, b.off[2u] = whether the unit exists
            const int nu = (cnt + 1) >> 1;
            const uint32_t dlo = (uint32_t)rpv, dhi = (uint32_t)((uint64_t)rpv >> 32);
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)dlo, 0);
            const uint32_t pN = (uint32_t)__builtin_amdgcn_readlane((int)dlo, G / 2);
            // A unit past the batch's last needs no select of its own: the clamped descriptor load
            // gives it the batch's end twice (no value pairs: every lane's offset is past every
            // range, zeros), its slot words' lane offsets lie past the slot range (zeros: the unit
            // goes into the lane offset, four loop-invariant registers, because the range check is
            // sure to see that one), and off = 0 sends every lane to its dummy slot whatever len
            // holds.
            const __amdgpu_buffer_rsrc_t rv = buf_rsrc(val + 2 * (int64_t)p0, (int)((pN - p0) * 16u));
            const __amdgpu_buffer_rsrc_t rl = buf_rsrc(lidx + 128 * (int64_t)un, nu * 256);
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                const uint32_t pa = (uint32_t)__builtin_amdgcn_readlane((int)dlo, u);
                const uint32_t pb = (uint32_t)__builtin_amdgcn_readlane((int)dlo, u + 1);
                const uint32_t cw = (uint32_t)__builtin_amdgcn_readlane((int)dhi, u);
                b.len[2 * u] = (int)(cw & 0xffu);
                b.len[2 * u + 1] = 0;
                b.off[2 * u] = u < nu ? 1 : 0;
                const int t = ln - (int)((cw >> 8) & 0xffu);
                const int vo = (uint32_t)t < pb - pa ? t * 16 : (1 << 30);   // (the unit's value pairs)
                const double2 tv = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rv, vo, (int)((pa - p0) * 16u), RW_AUX));
                b.v[u][0][0] = (T)tv.x;
                b.v[u][0][EPL - 1] = (T)tv.y;
                b.s[u][0] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rl, ln * 4 + u * 256, 0, RW_AUX);
            }
            return;
        }
        // the batch's entries from its first row's first pair; inside a batch the row pointers are
        // 32-bit offsets from it.  One resource per batch (its rows are consecutive): a row is an
        // SGPR offset into it, and the lanes past the row's (the unit's) last pair get an offset
        // past every range (no memory access, zeros), instead of a resource of their own per row
        const int64_t eb = readlane64(rpv, 0) & ~int64_t(1);
        const int bspan = (int)((readlane64(rpv, G) - eb + 1) & ~int64_t(1));
        const __amdgpu_buffer_rsrc_t rv = buf_rsrc(val + eb, bspan * ES);
        const __amdgpu_buffer_rsrc_t rl = buf_rsrc(lidx + eb, bspan * 2);
        // the lane's value pair and slot pair at byte offsets vo, lo (1 << 30: none) of the chunk that
        // starts `rel` entries into the batch
        auto load_pair = [&](int vo, int lo, int rel, T(&v)[EPL], uint32_t& s) {
            if constexpr (ES == 8) {
                const double2 t = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rv, vo, rel * ES, RW_AUX));
                v[0] = t.x;
                v[1] = t.y;
            } else {
                const float2 t = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(rv, vo, rel * ES, RW_AUX));
                v[0] = t.x;
                v[1] = t.y;
            }
            s = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rl, lo, rel * 2, RW_AUX);
        };
        if constexpr (F == PAIRS) {
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                // unit u = rows 2u, 2u+1 (a single row, or none, at the batch's end: lengths 0)
                const int64_t e0 = readlane64(rpv, 2 * u), e1 = readlane64(rpv, 2 * u + 1),
                              e2 = readlane64(rpv, 2 * u + 2);
                b.len[2 * u] = (int)(e1 - e0);
                b.len[2 * u + 1] = (int)(e2 - e1);
                const int off = (int)(e0 & 1);
                const int rel = (int)(e0 - eb) - off;
                b.off[2 * u] = off;
                const bool in = 2 * ln < (int)(e2 - e0) + off;
                const int vo = in ? 2 * ln * ES : (1 << 30), lo = in ? 2 * ln * 2 : (1 << 30);
                load_pair(vo, lo, rel, b.v[u][0], b.s[u][0]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int64_t e0 = readlane64(rpv, j), e1 = readlane64(rpv, j + 1);
                const int len = (int)(e1 - e0);
                b.len[j] = len;
                const int off = (int)(e0 & 1);
                const int rel = (int)(e0 - eb) - off;            // even: the row's first pair
                b.off[j] = off;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    const bool in = 2 * ln + CH * c < len + off;
                    const int vo = in ? (2 * ln + CH * c) * ES : (1 << 30), lo = in ? (2 * ln + CH * c) * 2 : (1 << 30);
                    load_pair(vo, lo, rel, b.v[j][c], b.s[j][c]);
                }
            }
        }
    };
    // Branch-free: entries outside the row (past its end, and the previous row's entry
    // in the first pair) are pointed at the lane's private dummy slot (MAXR - 64 + lane, q = 0),
    // so every row issues the same instructions and the compiler can interleave the G rows'
    // product and reduction chains (a branch would end the basic block).  The accumulator
    // updates stay in row order (consecutive rows share rays).
    T zx = T(0);                                  // this lane's share of the side sum, batches in order
    const bool first_lane = (ln & (GL - 1)) == 0;
    (void)first_lane;
    auto process = [&](RB& b) {
        T P[G];
        uint32_t k[G][NCH][EPL];
        uint32_t kb[G / 2][EPL];                  // (PAIRS, COMPACT) the second row's accumulator address
        if constexpr (VS) {
            // Four phases per batch, so the 24 LDS reads fly together instead of in short groups
            // with a wait each (two waves per SIMD: nobody else hides an LDS round trip):
            //   1 every address of the 4 units from their slot words;
            //   2 the 8 table reads, then the 16 q reads, back to back;
            //   3 the decode adds once the table entries are in, then each unit's FMAs behind a
            //     counted wait for that unit's q values (the LDS returns in order);
            //   4 the butterfly and the accumulator adds, below.
            // The empty asm statements pin an operand to its phase: they are ordered with the
            // sched_barriers, which the values themselves are not.  The arithmetic is unchanged
            // (entry 0 then entry 1 per lane and unit).
            const uint32_t dm = (uint32_t)(MAXR - 64 + ln) * (uint32_t)ES;
            uint32_t c8[G / 2][EPL];
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                const int la = b.len[2 * u];
                // (a unit that does not exist: every lane on its dummy, as the plan pads a unit's end)
                const uint32_t s = b.off[2 * u] ? b.s[u][0] : (dm | (dm << 16) | 0xc007c007u);
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const bool inA = 2 * ln + e < la;
                    const uint32_t sl = (e ? s >> 16 : s) & 0x3ff8u;
                    // the code's table offset ((31 - code) * 8): bits 14-18 of the word, or bits 30-31 | 0-2
                    c8[u][e] = (e ? __builtin_amdgcn_alignbit(s, s, 27) : s >> 11) & 0xf8u;
                    k[u][0][e] = inA ? sl : dm;
                    kb[u][e] = inA ? dm : sl;
                    asm volatile("" : "+v"(c8[u][e]), "+v"(k[u][0][e]), "+v"(kb[u][e]));
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            T tb[G / 2][EPL], qa[G / 2][EPL], qb[G / 2][EPL];
#pragma unroll
            for (int u = 0; u < G / 2; ++u)
#pragma unroll
                for (int e = 0; e < EPL; ++e)
                    tb[u][e] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + VTAB * ES + c8[u][e]);
            // (the table reads first, then the units' q reads in unit order: the counted waits of
            // phase 3 rely on it, and with every read an immediate offset from q at LDS address 0
            // the scheduler otherwise mixes the 24 and the waits become 14, 6, 3, 0)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    qa[u][e] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + k[u][0][e]);
                    qb[u][e] = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + kb[u][e]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                asm volatile("" : "+v"(tb[u][0]), "+v"(tb[u][EPL - 1]));
#pragma unroll
                for (int e = 0; e < EPL; ++e) b.v[u][0][e] = b.v[u][0][e] + tb[u][e];
            }
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                asm volatile("" : "+v"(qa[u][0]), "+v"(qb[u][0]), "+v"(qa[u][EPL - 1]), "+v"(qb[u][EPL - 1]));
                T pa = T(0), pb = T(0);
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const T v = b.v[u][0][e];
                    pa = fma_t(v, qa[u][e], pa);
                    pb = fma_t(v, qb[u][e], pb);
                }
                P[2 * u] = pa;
                P[2 * u + 1] = pb;
            }
        } else if constexpr (F == PAIRS) {
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                const int la = b.len[2 * u], lab = la + b.len[2 * u + 1];
                T pa = T(0), pb = T(0);
#pragma unroll
                for (int e = 0; e < EPL; ++e) {
                    const int pos = EPL * ln - b.off[2 * u] + e;
                    const bool inA = (uint32_t)pos < (uint32_t)la;
                    const bool in = (uint32_t)pos < (uint32_t)lab;
                    const uint32_t sl = e ? b.s[u][0] >> 16 : b.s[u][0] & 0xffffu;
                    const uint32_t dm = (uint32_t)(MAXR - 64 + ln) * (uint32_t)ES;
                    // the q reads go through the two accumulator addresses (q = 0 at the dummies;
                    // the q and accumulator offsets coincide): the row split costs a second q read
                    // instead of selects of the products
                    const uint32_t ka = inA ? sl : dm, kk = (in && !inA) ? sl : dm;
                    const T qa = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + ka);
                    const T qb = *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + kk);
                    pa = fma_t(b.v[u][0][e], qa, pa);
                    pb = fma_t(b.v[u][0][e], qb, pb);
                    k[u][0][e] = ka;
                    kb[u][e] = kk;
                }
                P[2 * u] = pa;
                P[2 * u + 1] = pb;
            }
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                T p = T(0);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        // slots are LDS byte offsets (the plan stores slot * sizeof(T)); pos0 is the lane's
                        // first entry in the row (-1: the previous row's last entry in the first pair)
                        const int pos0 = EPL * ln + CH * c - b.off[j];
                        const bool ok = e == 0 ? (uint32_t)pos0 < (uint32_t)b.len[j] : pos0 < b.len[j] - 1;
                        const uint32_t sl = e ? b.s[j][c] >> 16 : b.s[j][c] & 0xffffu;
                        k[j][c][e] = ok ? sl : (uint32_t)(MAXR - 64 + ln) * (uint32_t)ES;
                        p += b.v[j][c][e] * *reinterpret_cast<const T*>(reinterpret_cast<const char*>(qloc) + k[j][c][e]);
                    }
                P[j] = p;
            }
        }
        const T S = rows_sum_t<G>(P);             // lane l: z of row l / GL
        T zs = S;
        if constexpr (GK) {
            const T sa = ea * b.evv;              // row epilogue: zs = z - a*ev (two roundings)
            zs = S - sa;
        }
        {   // z out: each group's first lane, rows past cnt fall outside the range
            const __amdgpu_buffer_rsrc_t rz = buf_rsrc(zraw + b.r0, zraw ? b.cnt * ES : 0);
            buf_store(S, rz, row_off());
            if constexpr (GK) {
                const __amdgpu_buffer_rsrc_t ro = buf_rsrc(zout + b.r0, zout ? b.cnt * ES : 0);
                buf_store(zs, ro, row_off());
            }
        }
        // side: zs * x_true (other lanes: xv = 0), or zs^2 at the first lanes (rows past cnt: zs = 0)
        if constexpr (GK) {
            const T f = side_sq ? (first_lane ? zs : T(0)) : b.xv;
            zx = zx + zs * f;
        } else {
            zx = zx + zs * b.xv;
        }
        auto slot = [&](uint32_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ac) + off); };
        if constexpr (F != ROWS) {
#pragma unroll
            for (int u = 0; u < G / 2; ++u) {
                const T za = lane_bcast(zs, 2 * u * GL), zb = lane_bcast(zs, (2 * u + 1) * GL);
#pragma unroll
                for (int h = 0; h < 2; ++h) {         // the unit's first row, then its second
                    const T sj = h ? zb : za;
                    if constexpr (RAW) {
                        // read-add-write of the row's two entries per lane with ONE round trip: both
                        // reads, then both writes. Within one pixel row the slots are distinct, so
                        // only a lane whose two entries both sit on its dummy slot reads it twice
                        // (the dummy's value is never used): the same sums as one entry at a time.
                        T* p0 = slot(h ? kb[u][0] : k[u][0][0]);
                        T* p1 = slot(h ? kb[u][1] : k[u][0][1]);
                        const T o0 = *p0, o1 = *p1;
                        *p0 = fma_t(b.v[u][0][0], sj, o0);
                        *p1 = fma_t(b.v[u][0][1], sj, o1);
                    } else {
#pragma unroll
                        for (int e = 0; e < EPL; ++e) lds_add(slot(h ? kb[u][e] : k[u][0][e]), b.v[u][0][e] * sj);
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const T sj = lane_bcast(zs, j * GL);
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int e = 0; e < EPL; ++e) {
                        T* pa = slot(k[j][c][e]);
                        const T t = b.v[j][c][e] * sj;
                        if constexpr (RAW) *pa = *pa + t;
                        else lds_add(pa, t);
                    }
            }
        }
    };
    // Ring of D batches: while batch i is processed, batches i+1 .. i+D-1 are in flight and the
    // row pointers of batch i+D load.  The loop is unrolled by D so every ring index is static
    // (registers; a register copy of an in-flight load would force a wait), with one exit at the
    // bottom (a rotated loop with two exits had the compiler copy in-flight batches); an empty
    // batch is processed as a no-op (zero-length ranges, dummy slots).  sched_barrier: the
    // scheduler would sink the next batch's loads into the processing.
    RB b[D];
    int a[D], cn[D], un[D];
    int64_t r[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        next(a[i], cn[i], un[i]);
        r[i] = load_rp(a[i], cn[i], un[i]);
    }
    stage();                                      // (the gathers' waits leave the row pointers in flight)
#pragma unroll
    for (int i = 0; i < D - 1; ++i) issue(b[i], a[i], cn[i], r[i], un[i]);
    __syncthreads();                              // the staged q and the zeroed accumulators
    do {
#pragma unroll
        for (int t = 0; t < D; ++t) {
            // the row pointers of batch i+D first: issuing batch i+D-1 then waits only for its
            // own row pointers (loaded before batch i+D-2's entries), not for the entries
            const int ti = (t + D - 1) % D;
            next(a[t], cn[t], un[t]);
            r[t] = load_rp(a[t], cn[t], un[t]);
            issue(b[ti], a[ti], cn[ti], r[ti], un[ti]);
            __builtin_amdgcn_sched_barrier(0);
            // (compact pass: an empty batch, the round-up of the wave's batch count to a multiple
            // of D, is skipped by a wave-uniform branch: it would add zeros and store nothing)
            if (!VS || b[t].cnt > 0) process(b[t]);
            __builtin_amdgcn_sched_barrier(0);
        }
    } while (b[0].cnt > 0);
    if (zx_part) zx = wave_sum(zx);
    __syncthreads();
    // (the waves' side sums go through qloc, free once every wave has left the loop: an
    // array of their own would push the workgroup past half the LDS, one workgroup per CU)
    if (zx_part && ln == 0) qloc[wv] = zx;
    for (int k = threadIdx.x; k < nr; k += 64 * W) {
        T t = acc[0][k];
#pragma unroll
        for (int w = 1; w < W; ++w) t += acc[w][k];
        // the regions' partials are written once and read once, by the reduction: non-temporal stores
        // (fp64 pass + reduction 2.244 vs 2.252 ms, fp32 equal; profiles/r5_micro_part_nt_ab.txt)
        __builtin_nontemporal_store(t, &part[pb + k]);
    }
    if (zx_part) {
        __syncthreads();
        if (threadIdx.x == 0) {                   // waves in order
            T t = qloc[0];
#pragma unroll
            for (int w = 1; w < W; ++w) t += qloc[w];
            zx_part[g] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------
// plan (host, from B's CSR structure; once per operator)
// ------------------------------------------------------------------------------------------
namespace {
template <typename F>
void parallel_for(int64_t n, F f) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = std::max(1u, std::min(nt, 16u));
    if (n < 64 || nt == 1) {
        for (int64_t i = 0; i < n; ++i) f(i);
        return;
    }
    std::vector<std::thread> th;
    const int64_t step = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        const int64_t a = t * step, b = std::min<int64_t>(n, a + step);
        if (a >= b) break;
        th.emplace_back([=, &f]() {
            for (int64_t i = a; i < b; ++i) f(i);
        });
    }
    for (auto& t : th) t.join();
}

template <typename T>
T* upload(const std::vector<T>& v) {
    T* d = nullptr;
    const size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    if (hipMalloc(&d, bytes) != hipSuccess) throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
    if (!v.empty()) HGM_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
}  // namespace

// The pixel grid of B's rows: the whole tiled N x N grid (row_order), or a pixel shard of whole
// tile columns of one (row_grid: hgm_mat_row_slice, the multi-GPU path), whose stored positions
// are then shard-local.  Returns the grid (trivial when neither).
static PixOrder fused_grid(const hgm_mat* B) {
    const PixOrder& o = B->row_order;
    if (!o.trivial()) return (int64_t)o.N * o.N == B->rows ? o : PixOrder{};
    const PixOrder& g = B->row_grid;
    if (g.trivial() || g.super > 1 || B->rows % ((int64_t)std::max(g.tile, 1) * g.N) != 0) return PixOrder{};
    return g;
}

// Region (R x R pixel square) of every row of B (rows = pixels in B's stored order; for a shard
// the square grid is laid over the shard's N x W window of pixel columns).
static std::vector<int32_t> row_regions(const hgm_mat* B, int R, int64_t* nreg) {
    const PixOrder o = fused_grid(B);
    HGM_REQUIRE(!o.trivial() && o.N > 0, "fused A*(B*q): B's rows must be the pixels of a tiled N x N grid or a shard of it");
    const int N = o.N;
    const int64_t W = B->rows / N;                     // pixel columns (N for the whole grid)
    const int64_t nbr = (N + R - 1) / R, nbc = (W + R - 1) / R;
    *nreg = nbr * nbc;
    std::vector<int32_t> reg(B->rows);
    if (!B->row_order.trivial()) {
        const std::vector<int64_t> ref = pix_reference_of_stored(o);
        for (int64_t s = 0; s < B->rows; ++s) {
            const int64_t r = ref[s] % N, c = ref[s] / N;
            reg[s] = (int32_t)((c / R) * nbr + r / R);
        }
    } else {
        // shard: whole tile columns, tile x tile tiles in tile-column-major order, column-major
        // inside a tile (ops.hip pixel_rc without super-blocks), from the shard's first column
        const int64_t t = std::max(o.tile, 1), tpc = N / t;
        for (int64_t s = 0; s < B->rows; ++s) {
            const int64_t tl = s / (t * t), w = s % (t * t);
            const int64_t r = (tl % tpc) * t + w % t, c = (tl / tpc) * t + w / t;
            reg[s] = (int32_t)((c / R) * nbr + r / R);
        }
    }
    return reg;
}

// The row-wave plan: regions of R x R pixels, RW_WAVES waves per region.  Each wave gets a
// contiguous share (by entries) of the region's rows in stored order, as runs of consecutive
// rows; each entry gets its ray's index among the region's rays (sorted ray ids).
namespace {
constexpr int RW_SLOTS_MAX = 4096;                // rays + dummies the host build maps before it picks the slots
constexpr int RW_ROW_MAX = 255;                   // entries per pixel row (two chunks of 128, pairs)
// the fewest LDS ray slots of RwSlots that hold `worst` rays and the 64 dummies (0: none does)
template <int... Vs>
int rw_slots_for(Ints<Vs...>, int worst) {
    int best = 0;
    for (int v : {Vs...})
        if (worst <= v - 64 && (best == 0 || v < best)) best = v;
    return best;
}
}  // namespace

template <typename T, bool GK>
static bool fused_rw_launch(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P, const FusedArgs<T>& fa, bool dry);

// ------------------------------------------------------------------------------------------
// Device build of the row-wave plan's ray sets (HGM_OPT_FUSED_PLAN_DEV).  Per
// region, one workgroup marks the rays of the region's entries in an LDS bitmap over the ray
// space (atomic OR: order-free, so the set is the same whatever the schedule); a ray's slot is its
// rank among the set bits.  That is exactly the host build's sorted-unique ray list and
// map[ray] = index, so the plan's bytes are identical (tested).  The bitmap (and, in the fill
// pass, its per-word prefix counts) sit in dynamic LDS: ceil(m / 32) words each, so rays up to
// PLAN_DEV_MAX_M (C4: 272,271 rays, 68 KB).
// ------------------------------------------------------------------------------------------
namespace {
constexpr int PLAN_BS = 1024;
constexpr int64_t PLAN_DEV_MAX_M = int64_t(19) * 1024 * 32;   // 2 x 19 Ki words = 152 KB of LDS

// the region's entries (all its waves' runs), mark their rays in bm
__device__ __forceinline__ void plan_mark(uint32_t* bm, int nwords, const int32_t* __restrict__ wrun,
                                          const int2* __restrict__ runs, int W, const int64_t* __restrict__ rp,
                                          const int32_t* __restrict__ ci) {
    const int g = blockIdx.x;
    for (int i = threadIdx.x; i < nwords; i += PLAN_BS) bm[i] = 0u;
    __syncthreads();
    for (int u = wrun[g * W]; u < wrun[g * W + W]; ++u) {
        const int2 r = runs[u];
        const int64_t e1 = rp[r.x + r.y];
        for (int64_t e = rp[r.x] + threadIdx.x; e < e1; e += PLAN_BS) {
            const int32_t ray = ci[e];
            atomicOr(&bm[ray >> 5], 1u << (ray & 31));
        }
    }
    __syncthreads();
}

// exclusive prefix of v over the workgroup (fixed order), and the total
__device__ __forceinline__ int block_exscan(int v, int* sh, int* total) {
    const int ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (ln >= d) x += y;
    }
    if (ln == 63) sh[wv] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0;
        for (int w = 0; w < PLAN_BS / 64; ++w) {
            const int t = sh[w];
            sh[w] = a;
            a += t;
        }
        sh[PLAN_BS / 64] = a;
    }
    __syncthreads();
    *total = sh[PLAN_BS / 64];
    return sh[wv] + x - v;
}

__global__ __launch_bounds__(PLAN_BS) void k_plan_count(const int32_t* __restrict__ wrun, const int2* __restrict__ runs,
                                                        int W, const int64_t* __restrict__ rp,
                                                        const int32_t* __restrict__ ci, int nwords,
                                                        int32_t* __restrict__ cnt) {
    extern __shared__ uint32_t plan_lds[];
    __shared__ int sh[PLAN_BS / 64 + 1];
    plan_mark(plan_lds, nwords, wrun, runs, W, rp, ci);
    int c = 0;
    for (int i = threadIdx.x; i < nwords; i += PLAN_BS) c += __popc(plan_lds[i]);
    int tot = 0;
    (void)block_exscan(c, sh, &tot);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// ray_tab[reg_base[g] + rank] = ray (ascending), lidx[e] = rank(ci[e]) * es
__global__ __launch_bounds__(PLAN_BS) void k_plan_fill(const int32_t* __restrict__ wrun, const int2* __restrict__ runs,
                                                       int W, const int64_t* __restrict__ rp,
                                                       const int32_t* __restrict__ ci, int nwords,
                                                       const int64_t* __restrict__ reg_base,
                                                       int32_t* __restrict__ ray_tab, uint16_t* __restrict__ lidx,
                                                       int es) {
    extern __shared__ uint32_t plan_lds[];
    __shared__ int sh[PLAN_BS / 64 + 1];
    uint32_t* bm = plan_lds;
    uint32_t* pre = plan_lds + nwords;
    plan_mark(bm, nwords, wrun, runs, W, rp, ci);
    // words in contiguous per-thread chunks, so the exclusive scan of the chunk counts orders them
    const int cw = (nwords + PLAN_BS - 1) / PLAN_BS;
    const int w0 = min(nwords, (int)threadIdx.x * cw), w1 = min(nwords, w0 + cw);
    int c = 0;
    for (int i = w0; i < w1; ++i) c += __popc(bm[i]);
    int tot = 0;
    int a = block_exscan(c, sh, &tot);
    int32_t* rt = ray_tab + reg_base[blockIdx.x];
    for (int i = w0; i < w1; ++i) {
        pre[i] = (uint32_t)a;
        uint32_t b = bm[i];
        while (b) {
            const int k = __ffs(b) - 1;
            rt[a++] = i * 32 + k;
            b &= b - 1;
        }
    }
    __syncthreads();
    const int g = blockIdx.x;
    for (int u = wrun[g * W]; u < wrun[g * W + W]; ++u) {
        const int2 r = runs[u];
        const int64_t e1 = rp[r.x + r.y];
        for (int64_t e = rp[r.x] + threadIdx.x; e < e1; e += PLAN_BS) {
            const int32_t ray = ci[e];
            const uint32_t wd = bm[ray >> 5];
            const int rank = (int)pre[ray >> 5] + __popc(wd & ((1u << (ray & 31)) - 1u));
            lidx[e] = (uint16_t)(rank * es);
        }
    }
}
}  // namespace

// The band runs of k_fused_reduce_band from the plan's region ray lists (regions in order).
static void plan_bands(FusedPlan* P, const std::vector<int32_t>& ray_tab, const std::vector<int64_t>& reg_base) {
    const int64_t m = P->m, nreg = P->nreg, nband = (m + 63) / 64;
    std::vector<int32_t> cnt(nband + 1, 0);
    auto runs_of = [&](auto emit) {
        for (int64_t g = 0; g < nreg; ++g) {
            for (int64_t k = reg_base[g], k1 = reg_base[g + 1]; k < k1;) {
                const int32_t ray = ray_tab[k];
                const int64_t b = ray / 64;
                int64_t e = k + 1;
                while (e < k1 && ray_tab[e] == ray + (int32_t)(e - k) && ray_tab[e] / 64 == b) ++e;
                emit(b, make_int4((int)k, (int)(ray - b * 64), (int)(e - k), 0));
                k = e;
            }
        }
    };
    runs_of([&](int64_t b, int4) { cnt[b + 1]++; });
    for (int64_t b = 0; b < nband; ++b) cnt[b + 1] += cnt[b];
    std::vector<int4> run(std::max<int32_t>(cnt[nband], 1));
    std::vector<int32_t> fill(cnt.begin(), cnt.end() - 1);
    runs_of([&](int64_t b, int4 r) { run[fill[b]++] = r; });
    P->nband = nband;
    P->nrun = cnt[nband];
    P->band_ptr = upload(cnt);
    P->band_run = upload(run);
}

// ------------------------------------------------------------------------------------------
// Compact value stream (HGM_OPT_FUSED_VSTREAM, k_fused_rw COMPACT): built on the device from B's values
// and the plan's lidx, once per plan, after either build of the ray sets (so a host-built and a
// device-built plan hold the same bytes).  Every step is order-free or in a fixed order: the
// dictionary from a fixed-stride sample sorted on the host, integer counts, ranks by wave ballots
// in CSR order.
// ------------------------------------------------------------------------------------------
namespace {
constexpr int VS_CODES = 31;
constexpr int64_t VS_SAMPLE = int64_t(1) << 20;
// Take the compact streams when the pass's entry bytes (values, slots, row pointers or descriptors)
// shrink by at least this share.  The decode costs 3.3 % of the pass at C4 (empty dictionary, every
// value stored: 2,089 us against 2,023 us plain), the compact streams must save twice that, 6.5 % of the
// pass's bytes, and the entry streams are 86 % of those (10.17 of 11.81 GB): 7.6 %, rounded up.  With
// Siddon row lengths that is a coverage of about 12 % (C4: 29 % coded, entry bytes x 0.788).
// DESIGN.md §3.5.
constexpr double VS_MIN_SAVING = 0.08;

struct VsDict {
    uint64_t bits[32];            // ascending; code = index + 1
    int n;
};

__global__ void k_vs_sample(const double* __restrict__ val, int64_t stride, int64_t ns, uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ns) out[i] = (uint64_t)__double_as_longlong(val[i * stride]);
}

// code of a value (0: none), by binary search in the sorted dictionary
__device__ __forceinline__ int vs_code(const VsDict& d, uint64_t x) {
    int lo = 0, hi = d.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d.bits[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return (lo < d.n && d.bits[lo] == x) ? lo + 1 : 0;
}

// One wave per unit (unit_row: first row | single-row flag << 31): the unit's entries are CSR entries
// e0 .. e2, lane l taking e0 + l and e0 + l + 64.  pos[r]: the entry's position in the reordered unit.
struct VsUnit {
    int64_t e0;
    int n, nA;                    // entries, first row's entries
    int nCA, nEA, nEB, nCB;
    int code[2], pos[2];
    bool valid[2];
    uint64_t bits[2];
};
__device__ __forceinline__ VsUnit vs_unit(const VsDict& d, uint32_t ur, const int64_t* __restrict__ rp,
                                          const double* __restrict__ val, bool live) {
    VsUnit U;
    const int row = (int)(ur & 0x7fffffffu);
    const bool single = (ur >> 31) != 0;
    const int ln = threadIdx.x & 63;
    const int64_t e0 = live ? rp[row] : 0, e1 = live ? rp[row + 1] : 0, e2 = live ? (single ? e1 : rp[row + 2]) : 0;
    U.e0 = e0;
    U.n = (int)(e2 - e0);
    U.nA = (int)(e1 - e0);
    uint64_t m[4][2];
    const uint64_t lt = ((uint64_t)1 << ln) - 1;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = ln + 64 * r;
        U.valid[r] = i < U.n;
        U.bits[r] = U.valid[r] ? (uint64_t)__double_as_longlong(val[e0 + i]) : 0;
        U.code[r] = U.valid[r] ? vs_code(d, U.bits[r]) : 0;
        const bool isA = i < U.nA, cd = U.code[r] != 0;
        m[0][r] = __ballot(U.valid[r] && isA && cd);
        m[1][r] = __ballot(U.valid[r] && isA && !cd);
        m[2][r] = __ballot(U.valid[r] && !isA && !cd);
        m[3][r] = __ballot(U.valid[r] && !isA && cd);
    }
    U.nCA = __popcll(m[0][0]) + __popcll(m[0][1]);
    U.nEA = __popcll(m[1][0]) + __popcll(m[1][1]);
    U.nEB = __popcll(m[2][0]) + __popcll(m[2][1]);
    U.nCB = __popcll(m[3][0]) + __popcll(m[3][1]);
    const int base[4] = {0, U.nCA, U.nCA + U.nEA, U.nCA + U.nEA + U.nEB};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = ln + 64 * r;
        const bool isA = i < U.nA, cd = U.code[r] != 0;
        const int cls = isA ? (cd ? 0 : 1) : (cd ? 3 : 2);
        int rank = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (cls == q) rank = __popcll(m[q][r] & lt) + (r ? __popcll(m[q][0]) : 0);
        U.pos[r] = base[cls] + rank;
    }
    return U;
}

// per unit: its value pairs and descriptor word (bits 16-23: the unit's coded entries, summed and
// cleared by the host: one atomic per unit on one counter cost 0.1 s at C4); *nan += NaN values
__global__ __launch_bounds__(256) void k_vs_count(VsDict d, int64_t nunit, const uint32_t* __restrict__ unit_row,
                                                  const int64_t* __restrict__ rp, const double* __restrict__ val,
                                                  uint2* __restrict__ desc, unsigned long long* __restrict__ nan) {
    const int64_t un = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = un < nunit;
    const VsUnit U = vs_unit(d, live ? unit_row[un] : 0u, rp, val, live);
    int isnan_ = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r)
        isnan_ += (U.valid[r] && (U.bits[r] & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) ? 1 : 0;
    const int nans = __popcll(__ballot(isnan_ & 1)) + __popcll(__ballot(isnan_ & 2)) * 2;
    if (live && (threadIdx.x & 63) == 0) {
        const int nE = U.nEA + U.nEB;             // (no escapes: no pair, whatever the parity of nCA)
        const int np = nE ? ((U.nCA & 1) + nE + 1) >> 1 : 0;
        desc[un] = make_uint2((uint32_t)np, (uint32_t)U.nA | ((uint32_t)(U.nCA >> 1) << 8) |
                                                ((uint32_t)(U.nCA + U.nCB) << 16));
        if (nans) atomicAdd(nan, (unsigned long long)nans);
    }
}

// the unit's slot words and escape values (vals is zeroed beforehand: the positions that hold no
// escape); desc.x now holds the unit's first value pair
__global__ __launch_bounds__(256) void k_vs_fill(VsDict d, int64_t nunit, const uint32_t* __restrict__ unit_row,
                                                 const int64_t* __restrict__ rp, const double* __restrict__ val,
                                                 const uint16_t* __restrict__ lidx, const uint2* __restrict__ desc,
                                                 int maxr, uint32_t* __restrict__ slots, double* __restrict__ vals) {
    __shared__ uint16_t s16[4][128];
    __shared__ uint8_t c8[4][128];
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int64_t un = (int64_t)blockIdx.x * 4 + wv;
    const bool live = un < nunit;
    const VsUnit U = vs_unit(d, live ? unit_row[un] : 0u, rp, val, live);
    const uint16_t dm = (uint16_t)((maxr - 64 + ln) * 8);
    s16[wv][2 * ln] = dm;
    s16[wv][2 * ln + 1] = dm;
    c8[wv][2 * ln] = 0;
    c8[wv][2 * ln + 1] = 0;
    __syncthreads();
    const int64_t v0 = live ? 2 * (int64_t)desc[un].x - (U.nCA & ~1) : 0;   // value index of position 0
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (U.valid[r]) {
            s16[wv][U.pos[r]] = lidx[U.e0 + ln + 64 * r];
            c8[wv][U.pos[r]] = (uint8_t)U.code[r];
            if (U.code[r] == 0) vals[v0 + U.pos[r]] = __longlong_as_double((long long)U.bits[r]);
        }
    }
    __syncthreads();
    if (live) {
        // (the fields hold 31 - code: the table grows down from the dummies)
        const uint32_t a = s16[wv][2 * ln], b = s16[wv][2 * ln + 1], ca = 31u - c8[wv][2 * ln], cb = 31u - c8[wv][2 * ln + 1];
        slots[un * 64 + ln] = a | (b << 16) | (ca << 14) | ((cb & 3u) << 30) | (cb >> 2);
    }
}
}  // namespace

// Adds the compact streams to a finished fp64 row-pair plan when the options, the plan's shape and
// the operator's values allow it (otherwise the plan stays plain: today's streams, today's bits).
static void fused_plan_vstream(hgm_ctx* c, const hgm_mat* B, FusedPlan* P, const std::vector<int2>& runs, int worst) {
    const int mode = c->num.fused_vstream;
    const auto tv0 = std::chrono::steady_clock::now();
    P->nnz = B->nnz;
    if (!mode || P->elem != 8 || !P->rowpair || worst > P->maxr - 65 || B->nnz <= 0) return;
    const int room = std::min(VS_CODES, P->maxr - 65 - worst);   // codes the fullest region leaves slots for
    const int64_t nnz = B->nnz, nrun = (int64_t)runs.size();
    std::vector<int32_t> run_unit(std::max<int64_t>(nrun, 1), 0);
    int64_t nunit = 0;
    for (int64_t i = 0; i < nrun; ++i) {
        run_unit[i] = (int32_t)nunit;
        nunit += (runs[i].y + 1) / 2;
    }
    if (nunit <= 0 || nunit >= (int64_t(1) << 31) - 4) return;
    std::vector<uint32_t> unit_row(nunit);
    parallel_for(nrun, [&](int64_t i) {
        for (int k = 0; 2 * k < runs[i].y; ++k)
            unit_row[run_unit[i] + k] = (uint32_t)(runs[i].x + 2 * k) | (2 * k + 1 == runs[i].y ? 0x80000000u : 0u);
    });
    // the dictionary: the sample's most frequent patterns (seen at least twice; ties by bit pattern), finite,
    // normal and non-zero (0.0 + t must give t's bits)
    VsDict d{};
    uint64_t* samp_d = nullptr;
    uint32_t* unit_row_d = nullptr;
    unsigned long long* tot_d = nullptr;
    auto drop = [&](auto*& p) {
        if (p) (void)hipFree(p);
        p = nullptr;
    };
    auto cleanup = [&]() {
        drop(samp_d);
        drop(unit_row_d);
        drop(tot_d);
    };
    auto give_up = [&]() {       // the plan stays plain
        cleanup();
        drop(P->vs_desc);
        drop(P->vs_run_unit);
        drop(P->vs_table);
        drop(P->vs_slots);
        drop(P->vs_vals);
        P->vs_on = false;
        P->vs_pairs = 0;
        (void)hipGetLastError();
    };
    try {
        if (mode != 2) {
            const int64_t ns = std::min(nnz, VS_SAMPLE), stride = nnz / ns;
            if (hipMalloc(&samp_d, sizeof(uint64_t) * ns) != hipSuccess) return give_up();
            hipLaunchKernelGGL(k_vs_sample, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, c->stream,
                               (const double*)B->val, stride, ns, samp_d);
            HGM_HIP(hipGetLastError());
            std::vector<uint64_t> s(ns);
            HGM_HIP(hipMemcpyAsync(s.data(), samp_d, sizeof(uint64_t) * ns, hipMemcpyDeviceToHost, c->stream));
            HGM_HIP(hipStreamSynchronize(c->stream));
            std::sort(s.begin(), s.end());
            std::vector<std::pair<int64_t, uint64_t>> cand;   // (-count, bits)
            for (int64_t i = 0; i < ns;) {
                int64_t j = i;
                while (j < ns && s[j] == s[i]) ++j;
                const uint64_t ex = (s[i] >> 52) & 0x7ffu;
                if (j - i >= 2 && ex != 0 && ex != 0x7ffu) cand.emplace_back(-(j - i), s[i]);
                i = j;
            }
            std::sort(cand.begin(), cand.end());
            d.n = (int)std::min<size_t>(cand.size(), (size_t)room);
            for (int i = 0; i < d.n; ++i) d.bits[i] = cand[i].second;
            std::sort(d.bits, d.bits + d.n);
        }
        if (mode == 1 && d.n == 0) return give_up();
        P->vs_desc = upload(std::vector<uint2>(nunit + 1, make_uint2(0, 0)));
        P->vs_run_unit = upload(run_unit);
        unit_row_d = upload(unit_row);
        tot_d = upload(std::vector<unsigned long long>(2, 0ull));
        const unsigned grid = (unsigned)((nunit + 3) / 4);
        hipLaunchKernelGGL(k_vs_count, dim3(grid), dim3(256), 0, c->stream, d, nunit, (const uint32_t*)unit_row_d,
                           (const int64_t*)B->rp, (const double*)B->val, P->vs_desc, tot_d + 1);
        HGM_HIP(hipGetLastError());
        std::vector<uint2> desc(nunit + 1);
        unsigned long long tot[2] = {0, 0};
        HGM_HIP(hipMemcpyAsync(desc.data(), P->vs_desc, sizeof(uint2) * (nunit + 1), hipMemcpyDeviceToHost, c->stream));
        HGM_HIP(hipMemcpyAsync(tot, tot_d, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        HGM_HIP(hipStreamSynchronize(c->stream));
        int64_t pairs = 0, coded = 0;
        for (int64_t i = 0; i <= nunit; ++i) {     // value pairs per unit -> first pair (exclusive scan)
            const int64_t np = i < nunit ? desc[i].x : 0;
            desc[i].x = (uint32_t)pairs;
            pairs += np;
            coded += desc[i].y >> 16;
            desc[i].y &= 0xffffu;
        }
        tot[0] = (unsigned long long)coded;
        // entry bytes of the pass: plain 8 (value) + 2 (slot) per entry + 8 per row; compact 16 per
        // value pair + 256 (slots) + 8 (descriptor) per unit
        const double plain = 10.0 * (double)nnz + 8.0 * (double)B->rows;
        const double compact = 16.0 * (double)pairs + 264.0 * (double)nunit;
        const bool worth = compact <= (1.0 - VS_MIN_SAVING) * plain;
        P->vs_coded = (int64_t)tot[0];
        if (tot[1] != 0 || pairs >= (int64_t(1) << 32) || (mode == 1 && !worth)) return give_up();
        HGM_HIP(hipMemcpyAsync(P->vs_desc, desc.data(), sizeof(uint2) * (nunit + 1), hipMemcpyHostToDevice, c->stream));
        std::vector<double> table(32, 0.0);
        table[31] = -0.0;
        for (int i = 0; i < d.n; ++i) std::memcpy(&table[31 - (i + 1)], &d.bits[i], 8);
        P->vs_table = upload(table);
        if (hipMalloc(&P->vs_slots, sizeof(uint32_t) * 64 * (size_t)nunit) != hipSuccess ||
            hipMalloc(&P->vs_vals, 16 * (size_t)std::max<int64_t>(pairs, 1)) != hipSuccess)
            return give_up();                      // (no room for the second copy: the plain plan)
        HGM_HIP(hipMemsetAsync(P->vs_vals, 0, 16 * (size_t)std::max<int64_t>(pairs, 1), c->stream));
        hipLaunchKernelGGL(k_vs_fill, dim3(grid), dim3(256), 0, c->stream, d, nunit, (const uint32_t*)unit_row_d,
                           (const int64_t*)B->rp, (const double*)B->val, (const uint16_t*)P->lidx,
                           (const uint2*)P->vs_desc, P->maxr, P->vs_slots, P->vs_vals);
        HGM_HIP(hipGetLastError());
        HGM_HIP(hipStreamSynchronize(c->stream));
        P->nunit = nunit;
        P->vs_pairs = pairs;
        P->vs_on = true;
        cleanup();
        if (std::getenv("HGM_FUSED_VERBOSE"))
            std::fprintf(stderr, "[fused rw plan, value stream] %d codes cover %.4f of %lld entries; %lld units, values %lld B "
                         "(%.3f B/entry), slots %lld B; entry bytes %.4f of the plain streams'; %.3f s\n",
                         d.n, (double)P->vs_coded / (double)nnz, (long long)nnz, (long long)nunit, (long long)(16 * pairs),
                         16.0 * (double)pairs / (double)nnz, (long long)(256 * nunit), compact / plain,
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - tv0).count());
    } catch (...) {
        give_up();
        throw;
    }
}

// The one refusal a smaller region can cure (fused_ab_plan retries it with half the side); every
// other refusal of a plan (option shapes without a kernel, index ranges) goes straight to the
// two-pass path.
static const char* const kLdsCapacityMsg =
    "fused A*(B*q): a region is crossed by more rays than the LDS of its waves holds";

// The device part of the row-wave plan: ray sets, slots (lidx) and ray_tab by k_plan_count /
// k_plan_fill, then the ray-major reduction index by a counting sort of ray_tab on the host
// (slots in increasing order = regions in order, as the host build).
static FusedPlan* fused_plan_dev_finish(hgm_ctx* c, const hgm_mat* B, int R, bool rowpair, int es, int64_t nreg,
                                        int64_t maxlen, const std::vector<int32_t>& wrun,
                                        const std::vector<int2>& runs,
                                        std::chrono::steady_clock::time_point t0) {
    const int64_t m = B->cols, nnz = B->nnz;
    const int nwords = (int)((m + 31) / 32);
    FusedPlan* P = new FusedPlan;
    int32_t* cnt_d = nullptr;
    int worst_rays = 0;
    try {
        P->elem = es;
        P->region = R;
        P->rowpair = rowpair;
        P->maxlen = maxlen;
        P->nreg = nreg;
        P->m = m;
        P->wrun = upload(wrun);
        P->runs = upload(runs);
        if (hipMalloc(&cnt_d, sizeof(int32_t) * std::max<int64_t>(nreg, 1)) != hipSuccess)
            throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
        hipLaunchKernelGGL(k_plan_count, dim3((unsigned)nreg), dim3(PLAN_BS), sizeof(uint32_t) * nwords, c->stream,
                           (const int32_t*)P->wrun, (const int2*)P->runs, RW_WAVES, (const int64_t*)B->rp,
                           (const int32_t*)B->ci, nwords, cnt_d);
        HGM_HIP(hipGetLastError());
        std::vector<int32_t> cnt(nreg);
        HGM_HIP(hipMemcpyAsync(cnt.data(), cnt_d, sizeof(int32_t) * nreg, hipMemcpyDeviceToHost, c->stream));
        HGM_HIP(hipStreamSynchronize(c->stream));
        int worst = 0;
        for (int32_t v : cnt) worst = std::max(worst, (int)v);
        worst_rays = worst;
        const int maxr = rw_slots_for(RwSlots{}, worst);
        HGM_REQUIRE(maxr > 0, kLdsCapacityMsg);
        P->maxr = maxr;
        std::vector<int64_t> reg_base(nreg + 1, 0);
        for (int64_t g = 0; g < nreg; ++g) reg_base[g + 1] = reg_base[g] + cnt[g];
        const int64_t nslot = reg_base[nreg];
        HGM_REQUIRE(nslot < (int64_t(1) << 31), "fused A*(B*q): partial slots");
        P->nslot = nslot;
        P->reg_base = upload(reg_base);
        if (hipMalloc(&P->ray_tab, sizeof(int32_t) * std::max<int64_t>(nslot, 1)) != hipSuccess ||
            hipMalloc(&P->lidx, sizeof(uint16_t) * (nnz + 256)) != hipSuccess)
            throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
        HGM_HIP(hipMemsetAsync(P->lidx + nnz, 0, sizeof(uint16_t) * 256, c->stream));   // (the padding)
        hipLaunchKernelGGL(k_plan_fill, dim3((unsigned)nreg), dim3(PLAN_BS), 2 * sizeof(uint32_t) * nwords, c->stream,
                           (const int32_t*)P->wrun, (const int2*)P->runs, RW_WAVES, (const int64_t*)B->rp,
                           (const int32_t*)B->ci, nwords, (const int64_t*)P->reg_base, P->ray_tab, P->lidx, es);
        HGM_HIP(hipGetLastError());
        std::vector<int32_t> ray_tab(std::max<int64_t>(nslot, 1));
        HGM_HIP(hipMemcpyAsync(ray_tab.data(), P->ray_tab, sizeof(int32_t) * nslot, hipMemcpyDeviceToHost, c->stream));
        HGM_HIP(hipStreamSynchronize(c->stream));
        // ray-major reduction index: ray i's slots in region order (= increasing slot)
        std::vector<int64_t> rs_ptr(m + 1, 0);
        for (int64_t k = 0; k < nslot; ++k) rs_ptr[ray_tab[k] + 1]++;
        for (int64_t i = 0; i < m; ++i) rs_ptr[i + 1] += rs_ptr[i];
        std::vector<int32_t> rs_slot(std::max<int64_t>(nslot, 1));
        {
            std::vector<int64_t> fill(rs_ptr.begin(), rs_ptr.end() - 1);
            for (int64_t k = 0; k < nslot; ++k) rs_slot[fill[ray_tab[k]]++] = (int32_t)k;
        }
        P->rs_ptr = upload(rs_ptr);
        P->rs_slot = upload(rs_slot);
        plan_bands(P, ray_tab, reg_base);
        if (hipMalloc(&P->zx_part, sizeof(double) * std::max<int64_t>(nreg, 1)) != hipSuccess ||
            hipMalloc(&P->part, sizeof(double) * std::max<int64_t>(nslot, 1)) != hipSuccess)
            throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
        (void)hipFree(cnt_d);
        cnt_d = nullptr;
    } catch (...) {
        if (cnt_d) (void)hipFree(cnt_d);
        fused_plan_free(P);
        throw;
    }
    P->dev_built = true;
    P->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const bool have = es == 4 ? fused_rw_launch<float, true>(c, B, P, FusedArgs<float>{}, true)
                              : fused_rw_launch<double, false>(c, B, P, FusedArgs<double>{}, true);
    if (!have) {
        fused_plan_free(P);
        throw Error{HGM_E_ARG, "fused A*(B*q): no row-wave kernel for this plan's shape and the options"};
    }
    P->nwrun = (int64_t)runs.size();
    try {
        fused_plan_vstream(c, B, P, runs, worst_rays);
    } catch (...) {
        fused_plan_free(P);
        throw;
    }
    P->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (std::getenv("HGM_FUSED_VERBOSE"))
        std::fprintf(stderr, "[fused rw plan, device] region %d waves %d: %lld regions, %lld slots, max rays %d (LDS slots %d), %.3f s\n",
                     R, RW_WAVES, (long long)nreg, (long long)P->nslot, 0, P->maxr, P->build_s);
    return P;
}

static FusedPlan* fused_plan_build_rw(hgm_ctx* c, const hgm_mat* B, int R) {
    constexpr int W = RW_WAVES, G = RW_ROWS;
    const int es = B->dtype == HGM_F32 ? 4 : 8;       // slots as LDS byte offsets of T

    HGM_REQUIRE(B->cols < (int64_t(1) << 31) && B->rows < (int64_t(1) << 31), "fused A*(B*q): index range");
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = B->rows, m = B->cols, nnz = B->nnz;
    int64_t nreg = 0;
    const std::vector<int32_t> reg = row_regions(B, R, &nreg);
    // the ray sets on the device (no download of the column indices), or on the host (reference)
    const bool dev_build = c->num.fused_plan_dev && m <= PLAN_DEV_MAX_M && nnz > 0;
    std::vector<int64_t> rp(n + 1);
    std::vector<int32_t> ci(dev_build ? 1 : std::max<int64_t>(nnz, 1));
    HGM_HIP(hipMemcpy(rp.data(), B->rp, sizeof(int64_t) * (n + 1), hipMemcpyDeviceToHost));
    if (nnz && !dev_build) HGM_HIP(hipMemcpy(ci.data(), B->ci, sizeof(int32_t) * nnz, hipMemcpyDeviceToHost));
    int64_t maxlen = 0;
    for (int64_t s = 0; s < n; ++s) maxlen = std::max(maxlen, rp[s + 1] - rp[s]);
    HGM_REQUIRE(maxlen <= RW_ROW_MAX, "fused A*(B*q): a pixel row longer than the row-wave pass takes");
    // runs of consecutive stored rows of one region, per region in stored order
    std::vector<std::vector<int2>> rr(nreg);
    for (int64_t s = 0; s < n; ++s) {
        auto& v = rr[reg[s]];
        if (!v.empty() && v.back().x + v.back().y == s) ++v.back().y;
        else v.push_back(make_int2((int)s, 1));
    }
    // split each region's row sequence into W contiguous shares of about equal entries
    std::vector<std::vector<int2>> wr((size_t)nreg * W);
    parallel_for(nreg, [&](int64_t g) {
        int64_t tot = 0;
        for (const int2& r : rr[g]) tot += rp[r.x + r.y] - rp[r.x];
        int w = 0;
        int64_t done = 0;
        for (const int2& r : rr[g]) {
            for (int s = r.x; s < r.x + r.y; ++s) {
                while (w < W - 1 && done * W >= tot * (w + 1)) ++w;
                auto& v = wr[(size_t)g * W + w];
                if (!v.empty() && v.back().x + v.back().y == s) ++v.back().y;
                else v.push_back(make_int2(s, 1));
                done += rp[s + 1] - rp[s];
            }
        }
    });
    // Row pairs (k_fused_rw PAIRS): the kernel pairs rows 2i, 2i+1 of each run (batches start at even
    // offsets) and loads a pair as one chunk of 128 entries from its first row's first pair, so a
    // pair whose span (both rows + the alignment entry) exceeds 128 is not allowed: the run is cut
    // after the pair's first row, which then goes alone (C4: ~2.6 % of the pairs, ~4 cuts per wave).
    bool rowpair = c->num.fused_rowpair && maxlen + 1 <= 128;
    // does the unit (s, s+1) fit one chunk: both rows contiguous from s's first pair
    auto fits = [&](int64_t s) { return (rp[s + 2] - rp[s]) + (rp[s] & 1) <= 128; };
    // (rows so long that most pairs miss the chunk -- more than 64 runs in a wave after the cuts --
    // keep the plain row-wave plan: every unit would be a single row)
    if (rowpair) {
        std::vector<std::vector<int2>> wr1(wr.size());
        std::atomic<bool> over{false};
        parallel_for((int64_t)wr.size(), [&](int64_t i) {
            std::vector<int2>& out = wr1[(size_t)i];
            for (const int2& r : wr[(size_t)i]) {
                int s0 = r.x;
                const int end = r.x + r.y;
                int s = r.x;
                while (s < end) {
                    if (s + 1 < end && !fits(s)) {
                        out.push_back(make_int2(s0, s + 1 - s0));   // the run ends with row s alone
                        s0 = s + 1;
                        s = s + 1;
                    } else {
                        s += 2;
                    }
                }
                if (s0 < end) out.push_back(make_int2(s0, end - s0));
            }
            if (out.size() > 64) over = true;
        });
        if (over) rowpair = false;
        else wr.swap(wr1);
    }
    std::vector<int32_t> wrun((size_t)nreg * W + 1, 0);
    for (size_t i = 0; i < wr.size(); ++i) {
        HGM_REQUIRE(wr[i].size() <= 64, "fused A*(B*q): more than 64 row runs per wave");
        wrun[i + 1] = wrun[i] + (int32_t)wr[i].size();
    }
    std::vector<int2> runs(std::max<int32_t>(wrun.back(), 1));
    for (size_t i = 0; i < wr.size(); ++i) std::copy(wr[i].begin(), wr[i].end(), runs.begin() + wrun[i]);
    if (std::getenv("HGM_FUSED_VERBOSE")) {
        // batches per wave from the run table, and the empty batches a load ring of depth D adds: the
        // loop runs max(1, ceil(batches / D)) rounds of D batches (the compact pass skips their
        // processing, the other passes process them as no-ops)
        int64_t nb = 0, empty[5] = {0, 0, 0, 0, 0};
        for (size_t w = 0; w + 1 < wrun.size(); ++w) {
            int64_t b = 0;
            for (int i = wrun[w]; i < wrun[w + 1]; ++i) b += (runs[i].y + G - 1) / G;
            nb += b;
            for (int D = 2; D <= 4; ++D) empty[D] += std::max<int64_t>(1, (b + D - 1) / D) * D - b;
        }
        std::fprintf(stderr, "[fused rw plan] %lld waves, %lld batches; empty batches at ring depth 2: %lld, 3: %lld, 4: %lld\n",
                     (long long)wrun.size() - 1, (long long)nb, (long long)empty[2], (long long)empty[3], (long long)empty[4]);
    }
    if (dev_build) return fused_plan_dev_finish(c, B, R, rowpair, es, nreg, maxlen, wrun, runs, t0);
    // region ray sets and every entry's slot among them (a dense map per thread)
    std::vector<std::vector<int32_t>> rrays(nreg);
    std::vector<uint16_t> lidx(std::max<int64_t>(nnz, 1) + 256, 0);
    std::atomic<int> worst{0};
    {
        unsigned nt = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
        std::vector<std::thread> th;
        std::atomic<int64_t> nextg{0};
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&]() {
                std::vector<int32_t> map(m, -1);
                for (int64_t g; (g = nextg.fetch_add(1)) < nreg;) {
                    auto& rs = rrays[g];
                    for (const int2& r : rr[g])
                        for (int64_t e = rp[r.x]; e < rp[r.x + r.y]; ++e) rs.push_back(ci[e]);
                    std::sort(rs.begin(), rs.end());
                    rs.erase(std::unique(rs.begin(), rs.end()), rs.end());
                    int cur = worst.load();
                    while ((int)rs.size() > cur && !worst.compare_exchange_weak(cur, (int)rs.size())) {}
                    if (rs.size() > (size_t)RW_SLOTS_MAX - 64) continue;
                    for (size_t k = 0; k < rs.size(); ++k) map[rs[k]] = (int32_t)k;
                    for (const int2& r : rr[g])
                        for (int64_t e = rp[r.x]; e < rp[r.x + r.y]; ++e) lidx[e] = (uint16_t)(map[ci[e]] * es);
                    for (int32_t ray : rs) map[ray] = -1;
                }
            });
        for (auto& t : th) t.join();
    }
    const int maxr = rw_slots_for(RwSlots{}, worst.load());
    HGM_REQUIRE(maxr > 0, kLdsCapacityMsg);
    std::vector<int64_t> reg_base(nreg + 1, 0);
    for (int64_t g = 0; g < nreg; ++g) reg_base[g + 1] = reg_base[g] + (int64_t)rrays[g].size();
    const int64_t nslot = reg_base[nreg];
    HGM_REQUIRE(nslot < (int64_t(1) << 31), "fused A*(B*q): partial slots");
    std::vector<int32_t> ray_tab(std::max<int64_t>(nslot, 1));
    for (int64_t g = 0; g < nreg; ++g) std::copy(rrays[g].begin(), rrays[g].end(), ray_tab.begin() + reg_base[g]);
    // ray-major reduction index: ray i's slots in region order
    std::vector<int64_t> rs_ptr(m + 1, 0);
    for (int64_t g = 0; g < nreg; ++g)
        for (int32_t ray : rrays[g]) rs_ptr[ray + 1]++;
    for (int64_t i = 0; i < m; ++i) rs_ptr[i + 1] += rs_ptr[i];
    std::vector<int32_t> rs_slot(std::max<int64_t>(nslot, 1));
    {
        std::vector<int64_t> fill(rs_ptr.begin(), rs_ptr.end() - 1);
        for (int64_t g = 0; g < nreg; ++g)
            for (size_t r = 0; r < rrays[g].size(); ++r) rs_slot[fill[rrays[g][r]]++] = (int32_t)(reg_base[g] + r);
    }
    FusedPlan* P = new FusedPlan;
    try {
        P->elem = es;
        P->region = R;
        P->rowpair = rowpair;
        P->maxr = maxr;
        P->maxlen = maxlen;
        P->nreg = nreg;
        P->nslot = nslot;
        P->m = m;
        P->reg_base = upload(reg_base);
        P->wrun = upload(wrun);
        P->runs = upload(runs);
        P->ray_tab = upload(ray_tab);
        P->lidx = upload(lidx);
        if (hipMalloc(&P->zx_part, sizeof(double) * std::max<int64_t>(nreg, 1)) != hipSuccess)
            throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
        P->rs_ptr = upload(rs_ptr);
        P->rs_slot = upload(rs_slot);
        plan_bands(P, ray_tab, reg_base);
        if (hipMalloc(&P->part, sizeof(double) * std::max<int64_t>(nslot, 1)) != hipSuccess)
            throw Error{HGM_E_NOMEM, "fused plan: hipMalloc failed"};
    } catch (...) {
        fused_plan_free(P);
        throw;
    }
    P->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const bool have = es == 4 ? fused_rw_launch<float, true>(c, B, P, FusedArgs<float>{}, true)
                              : fused_rw_launch<double, false>(c, B, P, FusedArgs<double>{}, true);
    if (!have) {
        fused_plan_free(P);
        throw Error{HGM_E_ARG, "fused A*(B*q): no row-wave kernel for this plan's shape and the options"};
    }
    P->nwrun = (int64_t)runs.size();
    try {
        fused_plan_vstream(c, B, P, runs, worst.load());
    } catch (...) {
        fused_plan_free(P);
        throw;
    }
    P->build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (std::getenv("HGM_FUSED_VERBOSE"))
        std::fprintf(stderr, "[fused rw plan] region %d waves %d group %d: %lld regions, %lld slots, max rays %d (LDS slots %d), longest row %lld, %d runs, %.2f s\n",
                     R, W, G, (long long)nreg, (long long)nslot, worst.load(), maxr, (long long)maxlen, wrun.back(), P->build_s);
    return P;
}

// Whether w = A*(B*q) can run fused for this pair (B = A' value for value, tiled pixels or a shard
// of whole tile columns of them; fp64 or fp32).  On a communicator the caller all-reduces w, as it
// does A*(B*q) of the two-pass form.
bool fused_ab_eligible(const hgm_ctx* c, const hgm_mat* A, const hgm_mat* B) {
    if (!c->num.fused_ab || c->num.parity) return false;
    if (!A || !B || A->dtype != B->dtype) return false;
    if (A->dtype != HGM_F64 && A->dtype != HGM_F32) return false;
    if (!(B->transpose_of == A->uid || A->transpose_of == B->uid)) return false;
    return !fused_grid(B).trivial() && B->nnz > 0;
}

// The option tuple a plan is built for (a refused tuple is remembered per operator, so it is not
// re-planned on every solve, while any other tuple plans afresh)
static int64_t fused_key(const Numerics& nu) {
    return (int64_t)nu.fused_wregion | ((int64_t)nu.fused_plan_dev << 10) | ((int64_t)nu.fused_rowpair << 11) |
           ((int64_t)nu.fused_vstream << 14);
}

// The plan of B, built on first use (a failure to plan leaves the two-pass path in place).
const FusedPlan* fused_ab_plan(hgm_ctx* c, const hgm_mat* A, const hgm_mat* B) {
    if (!fused_ab_eligible(c, A, B)) return nullptr;
    hgm_mat* Bm = const_cast<hgm_mat*>(B);
    const Numerics& nu = c->num;
    const int64_t key = fused_key(nu);
    if (Bm->fused && Bm->fused_key != key) {          // options changed since the plan was built
        fused_plan_free(Bm->fused);
        Bm->fused = nullptr;
    }
    if (!Bm->fused && Bm->fused_failed_key != key) {   // (a refused tuple is not re-planned)
        try {
            // a region crossed by more rays than the LDS holds (many angles: the fan-beam
            // geometry over a full turn, ~7,400 rays per 32 x 32 region at 180 angles) is
            // retried with regions of half the side (about half the rays) before the pair
            // falls back to the two-pass path
            for (int R = nu.fused_wregion;; R /= 2) {
                try {
                    Bm->fused = fused_plan_build_rw(c, B, R);
                    break;
                } catch (const Error& e) {
                    if (e.code != HGM_E_ARG || e.msg != kLdsCapacityMsg || R / 2 < 16 || R % 2) throw;
                }
            }
            Bm->fused_key = key;
            Bm->fused_failed_key = -1;
        } catch (const Error& e) {
            if (e.code != HGM_E_ARG) throw;
            Bm->fused_failed_key = key;
        }
    }
    return Bm->fused;
}

// Launch the k_fused_rw instantiation for the plan and the options (dry: only report whether one
// exists; the plan is refused at build time when none does, so the two-pass path runs instead).
// Both answer from the shape lists beside the kernel.  GK = true: the row epilogue of the
// Golub-Kahan step, and every fp32 pass; it reads the plain streams of a compact plan.
template <typename T, bool GK>
static bool fused_rw_launch(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P, const FusedArgs<T>& fa, bool dry) {
    const bool side = fa.side_out != nullptr && (fa.xt != nullptr || fa.side_sq);
    auto go = [&](auto kernel, const int64_t* rp, const T* val, const uint16_t* lidx, VStream vs) {
        if (dry) return;
        launch(c, false, kernel, dim3((unsigned)P->nreg), dim3(64 * RW_WAVES), (const int64_t*)P->reg_base,
               (const int32_t*)P->ray_tab, (const int32_t*)P->wrun, (const int2*)P->runs, rp, val, lidx, fa.q, fa.zraw,
               (T*)P->part, side ? fa.xt : nullptr, side ? (T*)P->zx_part : nullptr, fa.ev, fa.easq, fa.zout,
               fa.side_sq ? 1 : 0, fa.pn, vs);
    };
    auto refuse = [&](const char* msg) -> bool {
        if (dry) return false;
        throw Error{HGM_E_ARG, msg};
    };
    const RwSlots slots{P->maxr, false};
    if (!P->rowpair) {
        // chunks per row: 128 entries, the first pair of which may start one entry early
        const RwChunks chunks{(int)((P->maxlen + 1 + 127) / 128), false};
        return dispatch([&](auto mr, auto nc) {
                   go(k_fused_rw<T, GK, mr, nc, RW_DEPTH, ROWS>, (const int64_t*)B->rp, (const T*)B->val,
                      (const uint16_t*)P->lidx, VStream{});
               }, slots, chunks) ||
               refuse("fused A*(B*q): no row-wave kernel for this plan and options");
    }
    if constexpr (sizeof(T) == 8 && !GK) {
        // the compact value stream: the plan's streams in place of B's values, lidx and row pointers,
        // and a load ring of its own depth (HGM_OPT_FUSED_VSDEPTH)
        if (P->vs_on)
            return dispatch([&](auto mr, auto d) {
                       go(k_fused_rw<T, GK, mr, 1, d, COMPACT>, (const int64_t*)nullptr, (const T*)P->vs_vals,
                          (const uint16_t*)P->vs_slots, VStream{P->vs_desc, P->vs_run_unit, P->vs_table});
                   }, slots, RwCompactDepths{c->num.fused_vsdepth, false}) ||
                   refuse("fused A*(B*q): no compact-stream kernel for this plan's shape and fused_vsdepth");
    }
    return dispatch([&](auto mr) {
               go(k_fused_rw<T, GK, mr, 1, RW_DEPTH, PAIRS>, (const int64_t*)B->rp, (const T*)B->val,
                  (const uint16_t*)P->lidx, VStream{});
           }, slots) ||
           refuse("fused A*(B*q): no row-pair kernel for this plan's shape and the options");
}

// Whether the Golub-Kahan form of the pass (row epilogue, side sum of squares; every fp32 pass)
// has a kernel for this plan.
bool fused_gk_ok(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P) {
    if (!P) return false;
    if (P->elem == 4) return fused_rw_launch<float, true>(c, B, P, FusedArgs<float>{}, true);
    return fused_rw_launch<double, true>(c, B, P, FusedArgs<double>{}, true);
}

__global__ void k_copy_sys(const double* __restrict__ src, double* dst) {
    if (threadIdx.x == 0) st_sys(dst, *src);
}
void copy_sys(hgm_ctx* c, const double* src, double* dst) {
    hipLaunchKernelGGL(k_copy_sys, dim3(1), dim3(64), 0, c->stream, src, dst);
    HGM_HIP(hipGetLastError());
}

// One pass over B (fa: internal.h FusedArgs): z = B*q, the row epilogue zs, w = A*zs, the side sum.
template <typename T>
bool fused_pass(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P, const FusedArgs<T>& fa) {
    HGM_REQUIRE((int)sizeof(T) == P->elem && (int)sizeof(T) == (B->dtype == HGM_F32 ? 4 : 8), "fused pass: dtype");
    const bool gk = fa.ev || fa.zout || fa.side_sq || sizeof(T) == 4;
    const bool side = fa.side_out != nullptr && (fa.xt != nullptr || fa.side_sq);
    hipEvent_t t0 = nullptr;
    timing_begin(c, KC_FUSED, &t0);
    if (gk) fused_rw_launch<T, true>(c, B, P, fa, false);
    else if constexpr (sizeof(T) == 8) fused_rw_launch<T, false>(c, B, P, fa, false);
    if (P->band_ptr && c->num.fused_reduce == 1) {
        const unsigned bgrid = (unsigned)std::max<int64_t>(1, (P->nband + BS / 64 - 1) / (BS / 64));
        launch(c, true, k_fused_reduce_band<T>, dim3(bgrid), dim3(BS), P->m, P->nband, (const int32_t*)P->band_ptr,
               (const int4*)P->band_run, (const T*)P->part, fa.w, (const T*)P->zx_part, (int)P->nreg,
               side ? fa.side_out : nullptr);
    } else {
        // one lane group per ray, no grid-stride cap (C4: 8,508 blocks; the 4,096 cap measured 5 us slower)
        const unsigned rgrid = (unsigned)std::max<int64_t>(1, (P->m * RG + BS - 1) / BS);
        // partials per lane: C4 ~14 (RB 16); rank g's shard of an 8-way cut ~1.8 (RB 4: the batch of
        // 16 issued 8x the loads it adds; round 6)
        const double ppl = (double)P->nslot / (double)std::max<int64_t>(1, P->m) / RG;
        dispatch([&](auto rb) {
            launch(c, true, k_fused_reduce<T, rb>, dim3(rgrid), dim3(BS), P->m, (const int64_t*)P->rs_ptr,
                   (const int32_t*)P->rs_slot, (const T*)P->part, fa.w, (const T*)P->zx_part, (int)P->nreg,
                   side ? fa.side_out : nullptr);
        }, ReduceBatches{ppl <= 4.0 ? 4 : ppl <= 8.0 ? 8 : 16});
    }
    HGM_HIP(hipGetLastError());
    // algorithmic bytes of the fused pass: B's CSR once (values, 32-bit indices, row pointers),
    // q read, z and w written (SURVEY.md §8(d)'s SpMV count for one pass over the operator), and
    // with the row epilogue its read of ev (the two-pass form's EPI_SUB operand)
    const double s = (double)sizeof(T);
    const double bytes = (s + 4.0) * (double)B->nnz + 8.0 * (B->rows + 1) + s * B->cols + s * B->rows + s * B->cols +
                         (fa.ev ? s * B->rows : 0.0);
    timing_end(c, KC_FUSED, t0, bytes);
    return side;
}
template bool fused_pass<double>(hgm_ctx*, const hgm_mat*, const FusedPlan*, const FusedArgs<double>&);
template bool fused_pass<float>(hgm_ctx*, const hgm_mat*, const FusedPlan*, const FusedArgs<float>&);


// Bq = B*q (n), ABq = A*(B*q) (m), one pass over B.
bool fused_ab(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P, const double* q, double* Bq, double* ABq,
              const double* xt, double* zx_out, const PendNorm<double>* pn) {
    FusedArgs<double> fa;
    fa.q = q;
    fa.zraw = Bq;
    fa.w = ABq;
    fa.xt = xt;
    fa.side_out = zx_out;
    if (pn && pn->np > 0) {
        HGM_REQUIRE(pn->hdev && pn->hring && pn->np <= MAX_PARTS, "fused A*(B*q): pending normalisation needs the row-wave pass");
        fa.pn = *pn;
    }
    return fused_pass<double>(c, B, P, fa);
}

// FNV-1a over the plan's arrays (hgm_fused_plan_info): two builds compare byte for byte
uint64_t fused_plan_checksum(hgm_ctx* c, const hgm_mat* B, const FusedPlan* P) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* dev, size_t bytes) {
        std::vector<unsigned char> v(bytes);
        if (bytes) HGM_HIP(hipMemcpy(v.data(), dev, bytes, hipMemcpyDeviceToHost));
        for (unsigned char b : v) h = (h ^ b) * 1099511628211ull;
    };
    int32_t nrun = 0;
    HGM_HIP(hipMemcpy(&nrun, P->wrun + P->nreg * RW_WAVES, sizeof(int32_t), hipMemcpyDeviceToHost));
    mix(P->wrun, sizeof(int32_t) * (P->nreg * RW_WAVES + 1));
    mix(P->runs, sizeof(int2) * nrun);
    mix(P->reg_base, sizeof(int64_t) * (P->nreg + 1));
    mix(P->ray_tab, sizeof(int32_t) * P->nslot);
    mix(P->lidx, sizeof(uint16_t) * B->nnz);
    mix(P->rs_ptr, sizeof(int64_t) * (P->m + 1));
    mix(P->rs_slot, sizeof(int32_t) * P->nslot);
    if (P->band_ptr) {
        mix(P->band_ptr, sizeof(int32_t) * (P->nband + 1));
        mix(P->band_run, sizeof(int4) * P->nrun);
    }
    if (P->vs_on) {                               // (large arrays in pieces: bounded host memory)
        auto mix_big = [&](const void* dev, size_t bytes) {
            const size_t step = size_t(256) << 20;
            for (size_t o = 0; o < bytes; o += step) mix((const char*)dev + o, std::min(step, bytes - o));
        };
        mix(P->vs_desc, sizeof(uint2) * (P->nunit + 1));
        mix(P->vs_run_unit, sizeof(int32_t) * nrun);
        mix(P->vs_table, sizeof(double) * 32);
        mix_big(P->vs_slots, sizeof(uint32_t) * 64 * (size_t)P->nunit);
        mix_big(P->vs_vals, 16 * (size_t)P->vs_pairs);
    }
    const int64_t meta[6] = {P->elem, P->region, RW_WAVES, P->maxr, P->maxlen, P->nslot};
    for (int64_t v : meta)
        for (int k = 0; k < 8; ++k) h = (h ^ (unsigned char)(v >> (8 * k))) * 1099511628211ull;
    (void)c;
    return h;
}
double fused_plan_build_seconds(const FusedPlan* P) { return P->build_s; }
int64_t fused_plan_slots(const FusedPlan* P) { return P->nslot; }
bool fused_plan_device_built(const FusedPlan* P) { return P->dev_built; }
void fused_plan_vstream_info(const FusedPlan* P, int* active, double* coverage, int64_t* value_bytes,
                             int64_t* plan_bytes) {
    if (active) *active = P->vs_on ? 1 : 0;
    if (coverage) *coverage = P->vs_on && P->nnz > 0 ? (double)P->vs_coded / (double)P->nnz : 0.0;
    if (value_bytes) *value_bytes = P->vs_on ? 16 * P->vs_pairs : 0;
    if (plan_bytes) {
        int64_t b = 4 * (P->nreg * RW_WAVES + 1) + 8 * P->nwrun + 8 * (P->nreg + 1) + 4 * P->nslot + 2 * (P->nnz + 256) +
                    8 * (P->m + 1) + 4 * P->nslot + 4 * (P->nband + 1) + 16 * P->nrun + 8 * P->nslot + 8 * P->nreg;
        if (P->vs_on) b += 8 * (P->nunit + 1) + 4 * P->nwrun + 256 + 256 * P->nunit + 16 * P->vs_pairs;
        *plan_bytes = b;
    }
}
}  // namespace hgm
