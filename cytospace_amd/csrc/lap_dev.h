// lap_dev.h -- device helpers shared by the LAP kernels (lap_jv.hip: the streaming kernels of every float32 solve; lap_chain_f32.hip:
// the float32 chain solver; lap_f64.hip: the float64 solver; lap_wide.hip, lap_wide_rr.hip, lap_wide_drv.hip: the wide solver; lap_exact.hip: the certificate and the
// exact option):
// the status block of a solve (LapStatus) with its counter and timer indices, order-preserving float keys, DPP wave reductions, the
// LDS-only barrier, the row-cache constants.
#pragma once
#include "cyto_common.h"
#include <math.h>
#include <stddef.h>

namespace cyto {

// Counters of a solve (LapStatus::counters): the first ten by every solver, the rest by the cached chain and the lazy augmentation.
enum { C_RT = 0, C_ARR, C_AUG_INIT, C_AUG_RELAX, C_AUGS, C_HOPS, C_FREE_CR, C_FREE_A1, C_FREE_A2, C_ROWS_READ, C_NCOUNTERS,
       C2_DENSE_REFRESH = C_NCOUNTERS, C2_AUG_SKIPPED, C2_NCOUNTERS,
       C2_AUG_DENSE = C2_NCOUNTERS, C2_AUG_SPARSE_INIT, C3_NCOUNTERS };
// Counters of the wide solver (LapStatus::wide)
enum { WC_ROUNDS = 0, WC_BIDS, WC_RETIRED, WC_ACTIVE_LEFT, WC_FREE_ARR, WC_DENSE_ARR, WC_DENSE_AUG, WC_AUG_ROUNDS, WC_AUG_PROCESSED,
       WC_TRIVIAL, WC_VERIFY_PASSES, WC_AUG_LAUNCHES, WC_N };
// What the wide kernels leave in LapStatus::timers: *_TICKS are 100 MHz ticks, the rest are counts.  A CYTO_WIDE_PROF build
// OVERLAYS WT_ARR_LAUNCHES .. WT_PAR_BATCHES and WT_PAR_DISCARDED with the tick split of wide_arr's chain rounds, so
// cyto_lap_info's wide_arr_launches, wide_scaled, wide_phases and wide_par_* are meaningless in such a build.
enum { WT_LIST_ROUNDS = 0, WT_LIST_TICKS, WT_CHAIN_ROUNDS, WT_CHAIN_TICKS,      // wide_arr: its list rounds and its chain rounds
       WT_DEALS, WT_ARR_SETUP_TICKS, WT_ARR_TAIL_TICKS,                         // wide_arr: re-deals of the chain rows; before / after the rounds
       WT_PAR_DISCARDED,                                                        // wide_aug<PAR>: searches run and thrown away
       WT_AUG_ROUNDS_TICKS, WT_AUG_VERIFY_TICKS, WT_AUG_FINISH_TICKS, WT_AUG_TRIVIAL_TICKS,     // wide_aug, by part of a search
       WT_ARR_LAUNCHES, WT_SCALED, WT_PHASES,                                   // launches of wide_arr; eps-scaled? (0 / 1); phases begun
       WT_PAR_BATCHES,                                                          // wide_aug<PAR>: batches of searches
       WT_N };

// The status block of one float32 / float64 solve: device memory that the kernels of both solvers write and the host drivers
// (lap_jv.hip, lap_f64.hip) zero before the solve and read back after it.
struct LapStatus {
    int nonfinite;                      // colred_partial: the cost holds a NaN or an infinity
    int status;                         // != 0: the solve failed (the finishers of the chain, the lazy and the wide kernels)
    double total;                       // the assignment's cost (finishers; exact_repair rewrites it)
    long long counters[C3_NCOUNTERS];   // C_* / C2_*
    int numfree;                        // rows still free before the augmentation (jv_chain2, wide_arr, the one-edge kernels)
    int wide_done;                      // searches done, wide solver (wide_aug and the one-edge kernels)
    int lazy_done;                      // searches completed by jv_aug_lazy (== numfree unless it gave up)
    int wide_embedded;                  // wide_aug<PAR>: 1 = the searches ran in the embedded form (the launch decides: lap_wide.hip, EMB_GATE)
    int ngroups;                        // runs of identical rows (rows_group_ids)
    int wide_aborted;                   // wide_aug<PAR>: searches ended early because they could no longer be committed (cyto_wide_aborted_searches)
    int pad1_[2];
    long long wide[WC_N];               // WC_*
    long long timers[WT_N];             // WT_*
    unsigned char arr[128];             // wide_arr's phase machine (lap_wide_rr.hip: ArrHead)
};
static_assert(sizeof(LapStatus) == 512, "LapStatus layout");
static_assert(offsetof(LapStatus, nonfinite) == 0 && offsetof(LapStatus, status) == 4 && offsetof(LapStatus, total) == 8, "LapStatus layout");
static_assert(offsetof(LapStatus, counters) == 16 && offsetof(LapStatus, numfree) == 128, "LapStatus layout");
static_assert(offsetof(LapStatus, wide_done) == 132 && offsetof(LapStatus, lazy_done) == 136, "LapStatus layout");
static_assert(offsetof(LapStatus, ngroups) == 144 && offsetof(LapStatus, wide) == 160, "LapStatus layout");
static_assert(offsetof(LapStatus, timers) == 256 && offsetof(LapStatus, arr) == 384, "LapStatus layout");
static_assert(C3_NCOUNTERS * 8 + 16 <= offsetof(LapStatus, numfree), "a new counter would overwrite numfree");
static_assert(WC_N * 8 + 160 <= offsetof(LapStatus, timers), "a new wide counter would overwrite the timers");
static_assert(WT_N == 16 && WT_N * 8 + 256 <= offsetof(LapStatus, arr), "a new timer would overwrite wide_arr's state");
// The kernels' argument blocks keep the block as char *misc (their mirror structs retype every pointer field)
__host__ __device__ __forceinline__ LapStatus *lap_status(char *misc) { return reinterpret_cast<LapStatus *>(misc); }

constexpr int KC = 64;             // cache slots per row (one per lane of a wave)
constexpr int KCU = 63;            // usable entries; slot 63 = { COLSENT, floor }
constexpr uint64_t KEYMAX = ~0ull;
constexpr uint32_t COLSENT = 0xFFFFFFFFu;

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));      // what a 16-byte raw buffer load returns

__device__ __forceinline__ uint32_t f2ord(float h) {
    const uint32_t b = __float_as_uint(h + 0.0f);  // +0.0f: -0 -> +0 so that equal floats get equal keys
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}
__device__ __forceinline__ uint64_t mkkey(float h, uint32_t lowbits) { return ((uint64_t)f2ord(h) << 32) | lowbits; }
__device__ __forceinline__ float key_val(uint64_t k) { return ord2f((uint32_t)(k >> 32)); }
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a < b ? b : a; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

struct K2 { uint64_t m1, m2; };  // two smallest keys of a set of DISTINCT keys (or KEYMAX)
__device__ __forceinline__ void k2_push(K2 &t, uint64_t k) {
    const uint64_t lo = umin64(t.m1, k), hi = umax64(t.m1, k);
    t.m1 = lo; t.m2 = umin64(t.m2, hi);
}
__device__ __forceinline__ void k2_merge(K2 &a, const K2 &b) {
    const uint64_t lo = umin64(a.m1, b.m1), hi = umax64(a.m1, b.m1);
    a.m2 = umin64(hi, umin64(a.m2, b.m2)); a.m1 = lo;
}

// DPP controls quad_perm[1,0,3,2] (0xB1), quad_perm[2,3,0,1] (0x4E), row_half_mirror (0x141),
// row_mirror (0x140): a butterfly inside each 16-lane row (merged sets are disjoint at every step).
template <int CTRL> __device__ __forceinline__ uint32_t dpp32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, CTRL, 0xF, 0xF, true);
}
template <int CTRL> __device__ __forceinline__ uint64_t dpp64(uint64_t x) {
    return ((uint64_t)dpp32<CTRL>((uint32_t)(x >> 32)) << 32) | dpp32<CTRL>((uint32_t)x);
}
__device__ __forceinline__ uint32_t readlane32(uint32_t x, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, l); }
__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l) {
    return ((uint64_t)readlane32((uint32_t)(x >> 32), l) << 32) | readlane32((uint32_t)x, l);
}
__device__ __forceinline__ uint32_t row_min_u32(uint32_t x) {
    x = umin32(x, dpp32<0xB1>(x)); x = umin32(x, dpp32<0x4E>(x));
    x = umin32(x, dpp32<0x141>(x)); x = umin32(x, dpp32<0x140>(x));
    return x;
}
// all lanes active; result is wave-uniform (scalar).  (Combining the four row minima with the gfx9 cross-row DPP controls
// row_bcast:15 / row_bcast:31 and one read-lane instead of four read-lanes + scalar mins was measured: 2 % slower.)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
    x = row_min_u32(x);
    return umin32(umin32(readlane32(x, 0), readlane32(x, 16)), umin32(readlane32(x, 32), readlane32(x, 48)));
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {
    x += dpp32<0xB1>(x); x += dpp32<0x4E>(x); x += dpp32<0x141>(x); x += dpp32<0x140>(x);
    return readlane32(x, 0) + readlane32(x, 16) + readlane32(x, 32) + readlane32(x, 48);
}
template <int CTRL> __device__ __forceinline__ void k2_step(K2 &t) {
    K2 o; o.m1 = dpp64<CTRL>(t.m1); o.m2 = dpp64<CTRL>(t.m2);
    k2_merge(t, o);
}
__device__ __forceinline__ void k2_row_allreduce(K2 &t) {
    k2_step<0xB1>(t); k2_step<0x4E>(t); k2_step<0x141>(t); k2_step<0x140>(t);
}
__device__ __forceinline__ K2 k2_wave_allreduce(K2 t) {
    k2_row_allreduce(t);
    K2 r; r.m1 = readlane64(t.m1, 0); r.m2 = readlane64(t.m2, 0);
#pragma unroll
    for (int row = 1; row < 4; row++) {
        K2 o; o.m1 = readlane64(t.m1, row * 16); o.m2 = readlane64(t.m2, row * 16);
        k2_merge(r, o);
    }
    return r;
}
__device__ __forceinline__ uint64_t min64_row_allreduce(uint64_t x) {
    x = umin64(x, dpp64<0xB1>(x)); x = umin64(x, dpp64<0x4E>(x));
    x = umin64(x, dpp64<0x141>(x)); x = umin64(x, dpp64<0x140>(x));
    return x;
}
__device__ __forceinline__ uint64_t min64_wave_allreduce(uint64_t x) {
    x = min64_row_allreduce(x);
    uint64_t r = readlane64(x, 0);
#pragma unroll
    for (int row = 1; row < 4; row++) r = umin64(r, readlane64(x, row * 16));
    return r;
}

// Barrier for LDS hand-offs only: waits for this wave's LDS traffic, NOT for its outstanding global
// stores/loads (a plain __syncthreads() carries s_waitcnt vmcnt(0): in the augmentation that made every
// step wait for the owner lane's global store to be acknowledged by HBM).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

}  // namespace cyto
