// lap_chain_f32.hip -- the float32 chain solver: the classic Jonker-Volgenant order after the column reduction, one dependent row
// scan after the other.  Not the default (the wide solver, lap_wide.hip, is): it runs under cyto_lap_opts.mode = 1 or any of the
// options chain_variant, augmentation, no_handover, inject_exceptions, group_state_global, aux_state_global.  Same operand order and
// the same lowest-index tie-breaking as the CPU oracle (oracle/jv_oracle_impl.h), so rowsol / colsol / u / v are bit-identical to it.
//
// Kernel plan (DESIGN.md section 4.1b has the exactness arguments and the measurements)
//   jv_chain2<CH, LDS_STATE> : REDUCTION TRANSFER + AUGMENTING ROW REDUCTION, a chain of dependent row scans.
//       One persistent 512-thread workgroup; a scan is served from the row's cache by wave 0 alone whenever the
//       cache certifies its top-2, otherwise the workgroup re-scans the row (refresh_row / refresh_row_stream).
//   jv_aug_lazy<LDS_STATE> (n > 5120) : AUGMENTATION with cache-certified scans and sparse search initialisation.
//   jv_aug2<CH, LDS_STATE> (n <= 5120, and taking over from jv_aug_lazy on deep searches) : dense augmentation,
//       per-column search state in registers.
// The column reduction, the runs of identical rows and the row caches it starts from are the driver's (lap_jv.hip), which calls
// chain_solve_batch (at the end of this file) through lap_chain_f32.h.
//
// Compile with -ffp-contract=off (build.py does): the arithmetic is subtract/compare only,
// but nothing may be re-associated.
#include "cyto_common.h"
#include "lap_dev.h"
#include "lap_chain.h"
#include "lap_chain_f32.h"
#include <math.h>
#include <algorithm>
#include <vector>
#include <stddef.h>
#include <string.h>

namespace cyto {

// The persistent chain kernels run one workgroup per PROBLEM: a batch of independent chunk LAPs is one launch with
// grid = batch size (consecutive workgroups land on consecutive XCDs, so the chains spread over the whole chip), each
// workgroup reading its own argument block.  One stream per chunk instead tops out at ~32 concurrent kernels
// (measured: 64 chunks on 64 streams took 3x as long as 32) and every 1-workgroup grid starts on XCD 0.

// ==========================================================================================
// float32 fast path ("v2").  Same arithmetic, same results, far fewer HBM row reads.
//
// Observation: during REDUCTION TRANSFER and AUGMENTING ROW REDUCTION the prices v[j] only ever
// DECREASE (RT subtracts a non-negative minimum, ARR only stores vj1_new when vj1_new < v[j1]),
// so every reduced cost h(i,j) = c[i][j] - v[j] only ever INCREASES.  Hence a row cache
//     C_i = { j : h(i,j) < F_i }  (at most KCU = 63 columns, with their raw c[i][j])  and the floor F_i
// built at any earlier time stays a valid certificate: every column outside C_i still has
// h >= F_i.  A later scan of row i only needs the cached columns: if the second-smallest
// recomputed cached value is < F_i, the cached top-2 IS the exact lexicographic top-2 of the
// whole row (bit-identical to the full scan).  Otherwise the row is re-scanned from HBM by the
// whole workgroup (and its cache rebuilt).  The caches of all rows are built once, right after
// the column reduction, by a full-chip streaming kernel (build_row_caches_wave).
//
// A cached step runs on ONE wave (lane = cache entry, lane 63 carries the floor): two coalesced
// 256-B loads, LDS gathers of v and colsol, three 32-bit DPP all-reduces on order-preserving float
// keys and a few scalar updates -- no barrier, no HBM row.
// ==========================================================================================
constexpr int BLOCK2 = 512;        // 8 waves: 256 VGPRs per lane for the column-resident state
constexpr int NW2 = BLOCK2 / 64;
enum { OP_EXIT = 0, OP_REFRESH = 1, OP_AUG = 2 };

// a wave's candidate for the next pick of the dense augmentation, with everything the step needs once it wins
struct __attribute__((aligned(16))) PickRec { uint64_t key; int32_t row; float h; float vjp; int32_t g; int32_t skip; int32_t srow; };   // srow: the stored row (row map applied)
struct Scratch2 {
    uint64_t m1[2][NW2], m2[2][NW2];
    int cnt[2][NW2];
    int cmd_op, cmd_row;
    double sum[NW2];
};

__device__ __forceinline__ K2 wg_k2(K2 t, Scratch2 &s, int &par) {
    t = k2_wave_allreduce(t);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s.m1[par][w] = t.m1; s.m2[par][w] = t.m2; }
    __syncthreads();
    K2 r; r.m1 = s.m1[par][lane & (NW2 - 1)]; r.m2 = s.m2[par][lane & (NW2 - 1)];
    k2_step<0xB1>(r); k2_step<0x4E>(r); k2_step<0x141>(r);   // 8 distinct partials per half-row: 3 steps only
    par ^= 1;
    r.m1 = readlane64(r.m1, 0); r.m2 = readlane64(r.m2, 0);
    return r;
}
__device__ __forceinline__ uint64_t wg_min64(uint64_t x, Scratch2 &s, int &par) {
    x = min64_wave_allreduce(x);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s.m1[par][w] = x;
    __syncthreads();
    uint64_t r = s.m1[par][lane & (NW2 - 1)];
    r = min64_row_allreduce(r);
    par ^= 1;
    return readlane64(r, 0);
}
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// sum over the waves of a wave-uniform int; *base = exclusive prefix for this wave
__device__ __forceinline__ int wg_sum_waves(int wave_val, Scratch2 &s, int &par, int *base) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s.cnt[par][w] = wave_val;
    __syncthreads();
    int tot = 0, b = 0;
#pragma unroll
    for (int i = 0; i < NW2; i++) { const int c = s.cnt[par][i]; if (i < w) b += c; tot += c; }
    par ^= 1;
    if (base) *base = b;
    return tot;
}
// exclusive scan of a per-thread int in thread order (set-up only; not on the hot path)
__device__ __forceinline__ int wg_exscan2(int x, Scratch2 &s, int &par, int *total) {
    const int lane = threadIdx.x & 63;
    int inc = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(inc, off); if (lane >= off) inc += y; }
    const int wtot = __shfl(inc, 63);
    int base = 0;
    *total = wg_sum_waves(wtot, s, par, &base);
    return base + inc - x;
}

struct CachePtrs {
    uint32_t *col;   // [n][KC]   slot 63: COLSENT
    float *val;      // [n][KC]   raw c[i][col]; slot 63: the floor (-inf = no usable cache)
};

// the column of slot sl of thread tid in a workgroup of BS threads (slot sl: quad sl / 4 of the thread, element sl % 4)
#define SLOT_COL(BS, sl) ((((sl) / 4) * (BS) + tid) * 4 + ((sl) % 4))

// One cost row through a bounds-checked buffer descriptor: lane `tid` gets 16 bytes of every
// 8 KiB chunk (a wave reads 1 KiB contiguous); bytes past the row pitch read as 0, so no branches.
template <int CH, int BS = BLOCK2>
__device__ __forceinline__ void load_row4(const float *__restrict__ cost, int64_t ld, int i, int n, int tid, float4 (&x)[CH]) {
    (void)n;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(cost + (int64_t)i * ld), 0, (int)(ld * 4), 0x00020000);
#pragma unroll
    for (int m = 0; m < CH; m++) {
        const u32x4_t t = __builtin_amdgcn_raw_buffer_load_b128(r, tid * 16, m * BS * 16, 0);
        x[m] = make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
    }
}
__device__ __forceinline__ float fmin_raw(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// The <= 63 entries of a rebuilt cache row are sorted by column (wave 0, bitonic network on 64 lanes; slot 63 keeps the
// floor): lane order is then column order, so "lowest column among equal reduced costs" -- the oracle's tie-break, and
// on CytoSPACE's duplicated spot rows ties at a reduced cost of exactly 0 are the rule -- is the lowest lane of a ballot
// instead of one more wave reduction per tie.
__device__ __forceinline__ void sort_cache_row(uint32_t *__restrict__ ccol, float *__restrict__ cval, float tau) {
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    uint32_t key = lane < KCU ? ccol[lane] : COLSENT;
    float val = lane < KCU ? cval[lane] : 0.0f;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t pk = __shfl_xor(key, j);
            const float pv = __shfl_xor(val, j);
            const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
            const bool sw = take_min ? (pk < key) : (pk > key);
            key = sw ? pk : key; val = sw ? pv : val;
        }
    }
    // unused slots and the floor slot all carry COLSENT and end up last, in no particular order: restore their values
    if (key == COLSENT) val = 0.0f;
    if (lane == KCU) { key = COLSENT; val = tau; }
    ccol[lane] = key; cval[lane] = val;
}

// Full scan of row i by the whole workgroup: exact two smallest keys of (c[i][j]-v[j], j) over all
// columns, plus a rebuilt cache for the row.  vreg = current prices of this thread's columns.
// delta adapts the cache threshold tau = umin + delta so that KCU/2..KCU columns qualify.
template <int CH>
__device__ __forceinline__ K2 refresh_row(int i, int n, int64_t ld, const float *__restrict__ cost,
                                          const float (&vreg)[CH * 4], uint64_t validm, uint32_t *__restrict__ cache_col,
                                          float *__restrict__ cache_val, float &delta, Scratch2 &s, int &par) {
    constexpr int NC = CH * 4;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    float4 x[CH];
    load_row4<CH>(cost, ld, i, n, tid, x);
#define HVAL(sl) (vec_get<float>(x[(sl) / 4], (sl) % 4) - vreg[sl])
    K2 loc; loc.m1 = KEYMAX; loc.m2 = KEYMAX;
#pragma unroll
    for (int sl = 0; sl < NC; sl++) {
        if ((validm >> sl) & 1) k2_push(loc, mkkey(HVAL(sl), (uint32_t)SLOT_COL(BLOCK2, sl)));
        if ((sl & 3) == 3) SCHED_FENCE();
    }
    const K2 g = wg_k2(loc, s, par);
    const float umin = key_val(g.m1);

    // threshold search (every thread computes the same sequence)
    float lo = 0.0f, hi = INFINITY, tau = INFINITY;
    int cnt = 0;
    bool okc = false;
    if (!(delta > 0.0f) || !(delta < 1e30f)) delta = 1e-3f;
    for (int it = 0; it < 24 && !okc; it++) {
        tau = umin + delta;
        uint32_t tc = 0;
#pragma unroll
        for (int sl = 0; sl < NC; sl++) { tc += (((validm >> sl) & 1) && HVAL(sl) < tau) ? 1u : 0u; if ((sl & 3) == 3) SCHED_FENCE(); }
        cnt = wg_sum_waves((int)wave_sum_u32(tc), s, par, nullptr);
        if (cnt > KCU) {
            hi = delta;
            const float mid = (lo > 0.0f) ? 0.5f * (lo + hi) : 0.5f * delta;
            if (!(mid < hi) || !(mid > lo)) break;   // cannot separate: too many ties just above umin
            delta = mid;
        } else if (cnt < KCU / 2 && cnt < n && delta < 1e30f) {
            lo = delta;
            const float mid = (hi < INFINITY) ? 0.5f * (lo + hi) : 2.0f * delta;
            if (hi < INFINITY && (!(mid < hi) || !(mid > lo))) { okc = true; break; }  // best separable threshold
            delta = mid;
        } else {
            okc = true;
        }
    }
    if (!okc || cnt > KCU) {
        // last resort: the largest threshold known to admit <= KCU columns (possibly none)
        if (lo > 0.0f) { delta = lo; tau = umin + lo; } else { tau = -INFINITY; }
    }
    // compaction: entries ordered by (wave, lane, slot); unused entries get the sentinel
    uint32_t tc = 0;
#pragma unroll
    for (int sl = 0; sl < NC; sl++) { tc += (((validm >> sl) & 1) && HVAL(sl) < tau) ? 1u : 0u; if ((sl & 3) == 3) SCHED_FENCE(); }
    int base = 0;
    cnt = wg_sum_waves((int)wave_sum_u32(tc), s, par, &base);
    if (cnt > KCU) { tau = -INFINITY; cnt = 0; tc = 0; }   // (cannot happen; keeps the cache valid regardless)
    uint32_t *ccol = cache_col + (int64_t)i * KC;
    float *cval = cache_val + (int64_t)i * KC;
    if (__ballot(tc != 0)) {
        // exclusive prefix of the per-lane counts inside the wave
        uint32_t inc = tc;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const uint32_t y = __shfl_up(inc, off); if (lane >= off) inc += y; }
        int pos = base + (int)(inc - tc);
        if (tc != 0) {
#pragma unroll
            for (int sl = 0; sl < NC; sl++) {
                if (((validm >> sl) & 1) && HVAL(sl) < tau) {
                    ccol[pos] = (uint32_t)SLOT_COL(BLOCK2, sl);
                    cval[pos] = vec_get<float>(x[sl / 4], sl % 4);
                    pos++;
                }
            }
        }
    }
    if (tid >= cnt && tid < KCU) { ccol[tid] = COLSENT; cval[tid] = 0.0f; }
    if (tid == KCU) { ccol[KCU] = COLSENT; cval[KCU] = tau; }
#undef HVAL
    __syncthreads();  // the rebuilt cache is complete before anyone may read it
    sort_cache_row(ccol, cval, tau);
    return g;
}

// Streaming variant of refresh_row for large n: no per-lane arrays.  The row and the prices come through
// bounds-checked buffer descriptors (whole quads stay in range: ld % 4 == 0 and v is followed by u in the
// workspace; the ragged tail is handled by the per-column validity compare) and the row is swept several times -- the first sweep from HBM, the rest
// from L2: top-2 keys, threshold search (count sweeps), per-lane counts, compaction.  Same cache contract
// as refresh_row.  VAUX = cache policy of the price loads: 0x10 (sc1, agent scope) inside the chain where
// wave 0 updates prices with agent-scope stores, 0 for the read-only build pass.
#define STREAM_SWEEP(BODY)                                                                               \
    for (int q = tid; q < nquad; q += BLOCK2) {                                                          \
        const u32x4_t xr_ = __builtin_amdgcn_raw_buffer_load_b128(rrow, q * 16, 0, 0);                   \
        const u32x4_t vr_ = __builtin_amdgcn_raw_buffer_load_b128(rv, q * 16, 0, VAUX);                  \
        const uint32_t c0_ = (uint32_t)q * 4;                                                            \
        { const float raw = __uint_as_float(xr_.x); const float h = raw - __uint_as_float(vr_.x); const uint32_t c = c0_;     if (c < (uint32_t)n) { BODY } } \
        { const float raw = __uint_as_float(xr_.y); const float h = raw - __uint_as_float(vr_.y); const uint32_t c = c0_ + 1; if (c < (uint32_t)n) { BODY } } \
        { const float raw = __uint_as_float(xr_.z); const float h = raw - __uint_as_float(vr_.z); const uint32_t c = c0_ + 2; if (c < (uint32_t)n) { BODY } } \
        { const float raw = __uint_as_float(xr_.w); const float h = raw - __uint_as_float(vr_.w); const uint32_t c = c0_ + 3; if (c < (uint32_t)n) { BODY } } \
    }
template <int VAUX>
__device__ __forceinline__ K2 refresh_row_stream(int i, int n, int64_t ld, const float *__restrict__ cost, const float *gv,
                                                 uint32_t *__restrict__ cache_col, float *__restrict__ cache_val, float &delta,
                                                 float &tau_guess, Scratch2 &s, int &par) {
    // Sweeps of the row: the first from HBM (top-2 keys AND the count below the previous row's floor -- neighbouring rows need
    // similar floors, and ANY floor that admits <= 63 columns makes a valid cache), then one per step of the threshold search from
    // L2.  Every counting sweep also keeps the thread's first two columns below the threshold, so the cache is written without
    // another sweep (a thread with more than two re-sweeps its own quads).  Typically one or two sweeps per row (six before:
    // the build was bound by L2, 10 TB/s of it for 1.5 TB/s of HBM at n = 50 000).
    const int tid = threadIdx.x, lane = tid & 63;
    const int nquad = (n + 3) >> 2;
    const __amdgpu_buffer_rsrc_t rrow = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(cost + (int64_t)i * ld), 0, (int)(ld * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(gv), 0, nquad * 16, 0x00020000);
    uint32_t tc = 0, hc0 = 0, hc1 = 0;                          // this thread's columns below the threshold: count, the first two
    float hr0 = 0.0f, hr1 = 0.0f;
#define STREAM_HIT(T) if (h < (T)) { if (tc == 0) { hc0 = c; hr0 = raw; } else if (tc == 1) { hc1 = c; hr1 = raw; } tc++; }
    K2 loc; loc.m1 = KEYMAX; loc.m2 = KEYMAX;
    const float tau0 = tau_guess;
    STREAM_SWEEP(k2_push(loc, mkkey(h, c)); STREAM_HIT(tau0))
    const K2 g = wg_k2(loc, s, par);
    const float umin = key_val(g.m1);
    int base = 0;
    int cnt = wg_sum_waves((int)wave_sum_u32(tc), s, par, &base);
    float tau = tau0;
    bool have = tau0 < INFINITY && cnt <= KCU && (cnt >= KCU / 2 || cnt >= n);      // the guess fits: done after one sweep
    if (have) delta = tau - umin;
    if (!have) {
        float lo = 0.0f, hi = INFINITY;
        bool okc = false;
        if (tau0 < INFINITY && tau0 > umin && cnt > 0) {          // scale the guess by how far its count was off
            const float d0 = tau0 - umin;
            if (cnt > KCU) { hi = d0; delta = d0 * fmaxf(0.0625f, 0.75f * (float)KCU / (float)cnt); }
            else { lo = d0; delta = d0 * fminf(16.0f, 0.75f * (float)KCU / (float)cnt); }
        }
        if (!(delta > 0.0f) || !(delta < 1e30f)) delta = 1e-3f;
        for (int it = 0; it < 24 && !okc; it++) {
            tau = umin + delta;
            tc = 0;
            STREAM_SWEEP(STREAM_HIT(tau))
            cnt = wg_sum_waves((int)wave_sum_u32(tc), s, par, &base);
            if (cnt > KCU) {
                hi = delta;
                const float mid = (lo > 0.0f) ? 0.5f * (lo + hi) : 0.5f * delta;
                if (!(mid < hi) || !(mid > lo)) break;
                delta = mid;
            } else if (cnt < KCU / 2 && cnt < n && delta < 1e30f) {
                lo = delta;
                const float mid = (hi < INFINITY) ? 0.5f * (lo + hi) : 2.0f * delta;
                if (hi < INFINITY && (!(mid < hi) || !(mid > lo))) { okc = true; break; }
                delta = mid;
            } else {
                okc = true;
            }
        }
        if (!okc || cnt > KCU) {
            // the largest threshold known to admit <= KCU columns (possibly none): counted once more, with its columns
            if (lo > 0.0f) { delta = lo; tau = umin + lo; } else { tau = -INFINITY; }
            tc = 0;
            STREAM_SWEEP(STREAM_HIT(tau))
            cnt = wg_sum_waves((int)wave_sum_u32(tc), s, par, &base);
            if (cnt > KCU) { tau = -INFINITY; cnt = 0; tc = 0; }
        }
    }
    tau_guess = tau > -INFINITY ? tau : INFINITY;
#undef STREAM_HIT
    uint32_t *ccol = cache_col + (int64_t)i * KC;
    float *cval = cache_val + (int64_t)i * KC;
    uint32_t inc = tc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t y = __shfl_up(inc, off); if (lane >= off) inc += y; }
    int pos = base + (int)(inc - tc);
    if (tc > 2) {
        STREAM_SWEEP(if (h < tau) { ccol[pos] = c; cval[pos] = raw; pos++; })
    } else {
        if (tc >= 1) { ccol[pos] = hc0; cval[pos] = hr0; }
        if (tc == 2) { ccol[pos + 1] = hc1; cval[pos + 1] = hr1; }
    }
    if (tid >= cnt && tid < KCU) { ccol[tid] = COLSENT; cval[tid] = 0.0f; }
    if (tid == KCU) { ccol[KCU] = COLSENT; cval[KCU] = tau; }
    __syncthreads();
    sort_cache_row(ccol, cval, tau);
    return g;
}

// Argument block of one problem (kernels get an array of them: one workgroup per problem).  Fields through an X-macro because
// the kernels read the block through a mirror struct whose pointers are typed as GLOBAL (LOAD_ARGS): pointers that are loaded from
// memory are generic to the compiler, and every access through them would be a FLAT instruction instead of a global one.
//   fws        float workspace: v[n] | u[n] | sumvd[n] | cassign[n] (= c[colsol[j]][j]) | 2n more
//   iws        int workspace: rowsol | colsol | matches | freerows | rtrows | pred | colgroup | ...   (n each)
//   cache_*    [n][KC] row caches;  misc: the status block (lap_dev.h: LapStatus)
//   rowgid     [n] duplicate-row group of every row (consecutive identical rows share an id)
//   rowmap     [n] stored row of every LAP row, or nullptr (row i is stored row i)
//   g_hbest / g_hstamp   [ngroups] scratch for gmode 2 (stamps zeroed)
//   gmode      0: no duplicate rows; 1: per-group state in LDS; 2: in global memory
//   auxlds     augmentation: cassign (f32) + colgroup (u16) per column also in LDS
//   aug_start  jv_aug2: first free row to augment (> 0: continues after jv_aug_lazy gave up)
#define CHAIN2_FIELDS(P, S)                                                                                             \
    S(int, n) S(int64_t, ld) P(const float, cost) P(float, fws) P(int32_t, iws) P(uint32_t, cache_col) P(float, cache_val)   \
    P(char, misc) P(int32_t, rowgid) P(const int32_t, rowmap) P(float, g_hbest) P(int32_t, g_hstamp)                        \
    S(int, ngroups) S(int, gmode) S(int, auxlds) S(int, aug_start)
#define F_PTR(T, name) T *name;
#define F_GPTR(T, name) __attribute__((address_space(1))) T *name;
#define F_VAL(T, name) T name;
#define F_COPY_PTR(T, name) a.name = (T *)g.name;
#define F_COPY_VAL(T, name) a.name = g.name;
struct Chain2Args { CHAIN2_FIELDS(F_PTR, F_VAL) };
struct Chain2ArgsG { CHAIN2_FIELDS(F_GPTR, F_VAL) };
static_assert(sizeof(Chain2Args) == sizeof(Chain2ArgsG), "mirror layout");
__device__ __forceinline__ Chain2Args load_args(const Chain2Args *__restrict__ batch) {
    const Chain2ArgsG g = reinterpret_cast<const Chain2ArgsG *>(batch)[blockIdx.x];
    Chain2Args a;
    CHAIN2_FIELDS(F_COPY_PTR, F_COPY_VAL)
    return a;
}

// L2-coherent (agent-scope, relaxed) accesses to global state
__device__ __forceinline__ float ld_f32(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t ld_u32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_f32(float *p, float x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// State accessors.  LDS_STATE: prices v (fp32) and colsol (u16, 0xFFFF = unassigned) live in LDS
// (n <= ~26k); otherwise they live in global memory and are accessed L2-coherently.
template <bool LDS_STATE> __device__ __forceinline__ float st_vget(const float *s_v, const float *gv, int j) {
    if constexpr (LDS_STATE) return s_v[j]; else return ld_f32(gv + j);
}
template <bool LDS_STATE> __device__ __forceinline__ void st_vset(float *s_v, float *gv, int j, float x) {
    if constexpr (LDS_STATE) s_v[j] = x; else st_f32(gv + j, x);
}
template <bool LDS_STATE> __device__ __forceinline__ int32_t st_csget(const uint16_t *s_cs, const int32_t *gcs, int j) {
    if constexpr (LDS_STATE) { const uint16_t c = s_cs[j]; return c == 0xFFFFu ? -1 : (int32_t)c; }
    else return ld_i32(gcs + j);
}
template <bool LDS_STATE> __device__ __forceinline__ void st_csset(uint16_t *s_cs, int32_t *gcs, int j, int32_t i) {
    if constexpr (LDS_STATE) s_cs[j] = (uint16_t)i; else st_i32(gcs + j, i);
}

template <int CH, bool LDS_STATE, int BS = BLOCK2>
__device__ __forceinline__ void load_vreg(const float *s_v, const float *gv, int n, int tid, float (&vreg)[CH * 4]) {
#pragma unroll
    for (int m = 0; m < CH; m++) {
        const int q = m * BS + tid;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q * 4 < n) {
            if constexpr (LDS_STATE) t = *reinterpret_cast<const float4 *>(s_v + q * 4);
            else {
                const int c = q * 4;
                t.x = ld_f32(gv + c);
                t.y = c + 1 < n ? ld_f32(gv + c + 1) : 0.f;
                t.z = c + 2 < n ? ld_f32(gv + c + 2) : 0.f;
                t.w = c + 3 < n ? ld_f32(gv + c + 3) : 0.f;
            }
        }
        vreg[m * 4 + 0] = t.x; vreg[m * 4 + 1] = t.y; vreg[m * 4 + 2] = t.z; vreg[m * 4 + 3] = t.w;
    }
}

template <int NWV = NW2>
__device__ __forceinline__ uint32_t wg_min_u32(uint32_t x, Scratch2 &s, int &par) {
    const uint32_t w0 = wave_min_u32(x);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *buf = reinterpret_cast<uint32_t *>(&s.cnt[par][0]);
    if (lane == 0) buf[w] = w0;
    lds_barrier();
    uint32_t r = buf[lane & (NWV - 1)];
    r = row_min_u32(r);
    par ^= 1;
    return readlane32(r, 0);
}

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float fmin3_raw(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// One augmentation (all threads, uniform control): dense Dijkstra search from `freerow`, price
// update, path flip.  Same pick rule as the oracle: lexicographic minimum of (d, assigned?, column)
// over the unscanned columns.  Per column the owning lane keeps, in VGPRs, the distance d (+inf
// once the column is scanned) and the price vm (-inf once scanned: every later relaxation of that
// column is then a no-op).  The arg-min is found in two steps: the minimum value first (one 32-bit all-reduce
// on order-preserving keys), then the column among the few lanes that hold that value.
//
// A step's cost on one CU is (a) the round trip of the picked row and (b) the VALU work of relaxing n columns, so
// the relaxation is as lean as the oracle's arithmetic allows: per PAIR of columns two packed subtractions
// (v_pk_add_f32 with negated operands: fl(fl(c - v) - h), the oracle's two roundings), per column one v_min_f32,
// per four columns two v_min3_f32 for the running minimum -- 2.5 VALU operations per column.
// No predecessor is tracked while relaxing (it cost a compare and two selects per column).  The oracle's pred[j] is the
// FIRST scan, in scan order and with the free row's initial scan before all others, whose candidate equals the final
// d[j] (a later equal candidate never replaces it: updates are strict); so every scan logs (row, h), every retired
// column logs the distance it was scanned at, and the <= ~40 columns of the augmenting path find their predecessors
// afterwards by re-evaluating the logged candidates for that one column (reconstruct_pred).
// LEAN (the usual configuration: the per-column auxiliaries and the duplicate-row group state are in LDS): the pick's look-ups
// are plain LDS reads with no global-memory alternative compiled in -- the alternatives cost a branch each and a
// `s_waitcnt vmcnt(0)` at every join.
template <int CH, bool LDS_STATE, int BS, bool LEAN>
__device__ __forceinline__ int chain_augment(int n, int64_t ld, const float *__restrict__ cost, float *gv, float2 *sd,
                                             float *cassign, int32_t *rowsol, int32_t *gcolsol, int32_t *slog_row, float *slog_h,
                                             float *s_v, uint16_t *s_cs, int freerow, uint64_t validm, Scratch2 &s, int &par,
                                             long long &c_relax, long long &c_hops, long long &c_skipped, int gmode,
                                             const int32_t *rowgid, int32_t *colgroup, float *hb, int32_t *hs, int stamp, float *s_ca,
                                             uint16_t *s_cg, PickRec (*rec)[NW2], const int32_t *__restrict__ rowmap) {
    constexpr int NC = CH * 4;
    constexpr int NWV = BS / 64;
    const int tid = threadIdx.x;
    // Column state as two register VECTORS: a slot that is only known at run time, but is the same for the whole wave
    // (the retired column's, the picked column's), is then read or written with indirect register addressing
    // (s_set_gpr_idx / v_movrel: a handful of instructions) instead of a compare-and-select per slot.  The hardware indexes
    // at most 32 registers that way; beyond (NC > 32) the select chains remain.
    typedef float fvec __attribute__((ext_vector_type(NC)));
    constexpr bool VEC = NC <= 32;
    fvec vmV, dV;
    float cm[CH];
    // LDS views with their address space spelled out: through plain (generic) pointers that may also be null or point to
    // global memory the compiler emits FLAT loads, which take the long way round (measured: ~1000 cycles for the four
    // look-ups of a step)
    typedef __attribute__((address_space(3))) float lds_f32;
    typedef __attribute__((address_space(3))) uint16_t lds_u16;
    typedef __attribute__((address_space(3))) int32_t lds_i32;
    lds_f32 *const l_v = (lds_f32 *)s_v;
    lds_u16 *const l_cs = (lds_u16 *)s_cs;
    lds_f32 *const l_ca = (lds_f32 *)s_ca;
    lds_u16 *const l_cg = (lds_u16 *)s_cg;
    lds_f32 *const l_hb = (lds_f32 *)hb;
    lds_i32 *const l_hs = (lds_i32 *)hs;
    typedef __attribute__((address_space(3))) PickRec lds_rec;
    lds_rec *const l_rec = (lds_rec *)&rec[0][0];          // [2][NW2]
#define VM(sl) vmV[sl]
#define DR(sl) dV[sl]
    {
        float v0[NC];
        load_vreg<CH, LDS_STATE, BS>(s_v, gv, n, tid, v0);
#pragma unroll
        for (int sl = 0; sl < NC; sl++) VM(sl) = v0[sl];
    }
    uint64_t assignedm = 0, scannedm = 0, readym = 0;
#pragma unroll
    for (int sl = 0; sl < NC; sl++)
        if (((validm >> sl) & 1) && st_csget<LDS_STATE>(s_cs, gcolsol, SLOT_COL(BS, sl)) >= 0) assignedm |= (1ull << sl);
    {
        float4 x[CH];
        load_row4<CH, BS>(RBASE(cost, rowmap, freerow, ld), ld, freerow, n, tid, x);
#pragma unroll
        for (int sl = 0; sl < NC; sl++) {
            const bool ok = (validm >> sl) & 1;
            DR(sl) = ok ? vec_get<float>(x[sl / 4], sl % 4) - VM(sl) : INFINITY;
            VM(sl) = ok ? VM(sl) : -INFINITY;
        }
    }
#pragma unroll
    for (int m = 0; m < CH; m++) cm[m] = fmin_raw(fmin3_raw(DR(m * 4), DR(m * 4 + 1), DR(m * 4 + 2)), DR(m * 4 + 3));
    bool have = false;
    float curmin = 0.0f;
    int endofpath = -1;
    int nlog = 0;            // scans logged so far in this search (uniform)
    const int lane = tid & 63, wave = tid >> 6;
    for (;;) {
        // ---- pick: smallest d; among equal d an unassigned column first, then the lowest column.  ONE workgroup
        // exchange per step: every wave reduces its own columns to a candidate (value, then column among the lanes that
        // hold that value: two DPP all-reduces, no barrier), looks up what the step needs if that candidate wins (owner
        // row, its offset h, the duplicate-row skip test: independent broadcast LDS reads) and posts the record; after the
        // barrier every wave reduces the eight 64-bit keys and reads the winner's record. ----
        float lm = cm[0];
#pragma unroll
        for (int m = 1; m < CH; m++) lm = fmin_raw(lm, cm[m]);
        const uint32_t wmin = wave_min_u32(f2ord(lm));
        const float dminw = ord2f(wmin);
        uint32_t lk = 0xFFFFFFFFu;
        const uint64_t holders = __ballot(lm == dminw && dminw < INFINITY);
        bool one_group = false;
        int mg = CH - 1;
        if (VEC && __builtin_popcountll(holders) == 1) {
            // the usual case: ONE lane of the wave holds the minimum, in ONE of its groups of four.  (Two groups of the lane at the
            // same value go the general way below: an unassigned column of the later group beats an assigned one of the first.)
            int ng = cm[CH - 1] == dminw ? 1 : 0;
#pragma unroll
            for (int m = CH - 2; m >= 0; m--) { const bool eq = cm[m] == dminw; mg = eq ? m : mg; ng += eq ? 1 : 0; }   // first group that holds the value
            one_group = __builtin_amdgcn_readlane(ng, (int)__builtin_ctzll(holders)) == 1;
        }
        if (one_group) {
            // The group (found with CH compares) is broadcast, the four slots are fetched with indirect addressing, the holder picks among them.
            const int hl = (int)__builtin_ctzll(holders);
            const int mgu = __builtin_amdgcn_readlane(mg, hl);                   // wave-uniform
            if (lm == dminw) {
#pragma unroll
                for (int e = 3; e >= 0; e--) {
                    const int sl = mgu * 4 + e;
                    const float de = dV[sl];
                    const uint32_t key = (uint32_t)(((mgu * BS + tid) << 2) + e) | (uint32_t)((assignedm >> sl) & 1) << 31;
                    lk = de == dminw ? umin32(lk, key) : lk;
                }
            }
        } else if (lm == dminw && dminw < INFINITY) {
#pragma unroll
            for (int m = 0; m < CH; m++) {
                if (cm[m] == dminw) {
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        const int sl = m * 4 + e;
                        if (DR(sl) == dminw)
                            lk = umin32(lk, (uint32_t)SLOT_COL(BS, sl) | (((assignedm >> sl) & 1) ? 0x80000000u : 0u));
                    }
                }
            }
        }
        const uint32_t wlk = wave_min_u32(lk);
        {
            int32_t iw = -1, gw = 0, skipw = 0, sroww = 0;
            float hw = 0.0f, vjpw = 0.0f;
            if (wlk != 0xFFFFFFFFu && (wlk & 0x80000000u)) {          // (wave-uniform) an assigned column: its owner row
                const int jpw = (int)(wlk & 0x7FFFFFFFu);
                float cipw;                                                     // c[i][jp]
                if constexpr (LEAN) { cipw = l_ca[jpw]; gw = (int)l_cg[jpw]; }
                else { cipw = s_ca ? l_ca[jpw] : ld_f32(cassign + jpw); gw = gmode ? (s_cg ? (int)l_cg[jpw] : ld_i32(colgroup + jpw)) : 0; }
                if constexpr (LDS_STATE) { const uint16_t c16 = l_cs[jpw]; iw = c16 == 0xFFFFu ? -1 : (int32_t)c16; vjpw = l_v[jpw]; }
                else { iw = ld_i32(gcolsol + jpw); vjpw = ld_f32(gv + jpw); }
                hw = (cipw - vjpw) - dminw;
                // the stored row of the owner (row map): looked up here, by every wave for its own candidate and next to the LDS
                // look-ups, not after the exchange -- there it was a dependent round trip to L2 in front of every row fetch
                sroww = iw;
                if (rowmap && iw >= 0) sroww = rowmap[__builtin_amdgcn_readfirstlane(iw)];
                // Exact skip for duplicated rows: if a bitwise identical row was already scanned in THIS search with an
                // offset hb >= h, every relaxation through row i is a no-op: fl(x - h) >= fl(x - hb) >= d[j] for every
                // unscanned column (prices do not change during a search and d only decreases).  The column is retired
                // exactly as usual, only the row read and the relaxation sweep are elided.
                if (gmode) {
                    float hbv; int hsv;
                    if (LEAN || gmode == 1) { hbv = l_hb[gw]; hsv = l_hs[gw]; }
                    else { hbv = ld_f32(hb + gw); hsv = ld_i32(hs + gw); }
                    skipw = ((hsv == stamp) && (hw <= hbv)) ? 1 : 0;
                }
            }
            if (lane == 0) {
                lds_rec *const dst = l_rec + par * NW2 + wave;
                dst->key = ((uint64_t)wmin << 32) | wlk; dst->row = iw; dst->h = hw; dst->vjp = vjpw; dst->g = gw; dst->skip = skipw; dst->srow = sroww;
            }
        }
        lds_barrier();
        uint64_t k8 = l_rec[par * NW2 + (lane & (NWV - 1))].key;
        uint64_t kmin = k8;
        kmin = umin64(kmin, dpp64<0xB1>(kmin)); kmin = umin64(kmin, dpp64<0x4E>(kmin));
        if constexpr (NWV > 4) kmin = umin64(kmin, dpp64<0x141>(kmin));
        kmin = readlane64(kmin, 0);
        const int wstar = (int)__builtin_ctzll(__ballot(k8 == kmin)) & (NWV - 1);     // keys of distinct waves are distinct columns
        const lds_rec *const win = l_rec + par * NW2 + wstar;
        const int32_t rw_row = win->row, rw_g = win->g, rw_skip = win->skip, rw_srow = win->srow;
        const float rw_h = win->h, rw_vjp = win->vjp;
        par ^= 1;
        const float dmin = ord2f((uint32_t)(kmin >> 32));
        const uint32_t g = (uint32_t)kmin;
        if (g == 0xFFFFFFFFu || !(dmin < INFINITY)) return CYTO_ERR_INTERNAL;
        const int jp = (int)(g & 0x7FFFFFFFu);
        if (!have || dmin != curmin) { readym |= scannedm; curmin = dmin; have = true; }
        if (!(g & 0x80000000u)) { endofpath = jp; break; }
        const int i = __builtin_amdgcn_readfirstlane(rw_row);
        const float h = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(rw_h)));
        const float vjp = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(rw_vjp)));
        const bool skip = __builtin_amdgcn_readfirstlane(rw_skip) != 0;
        if (gmode && !skip && lane == 0) {
            // the group's new best offset.  Every wave posts the same value: its own later look-ups (program order) see it
            // without another barrier, whichever wave is first
            const int grp = rw_g;
            if (LEAN || gmode == 1) { l_hb[grp] = h; l_hs[grp] = stamp; }
            else { st_f32(hb + grp, h); st_i32(hs + grp, stamp); }
        }
        float4 x[CH];
        if (!skip) {
            const int srow = __builtin_amdgcn_readfirstlane(rw_srow);
            load_row4<CH, BS>(cost + ((int64_t)srow - i) * ld, ld, i, n, tid, x);
            // scan log (after the loads in program order: a store does not hold them up); one store instruction of the last wave
            if (tid >= BS - 2) {
                if (tid == BS - 2) st_i32(slog_row + nlog, i);
                else st_f32(slog_h + nlog, h);
            }
            nlog++;
        }
        {   // retire column jp: remember v+d (price update) and d (predecessor search), mask the column out.
            // The slot is wave-uniform: a scalar branch per slot instead of two selects per slot.
            const int q = jp >> 2;
            const int sj = (q / BS) * 4 + (jp & 3);   // uniform
            const bool own = (q % BS) == tid;
            if (own) { scannedm |= (1ull << sj); sd[jp] = make_float2(vjp + dmin, dmin); }
            if constexpr (VEC) {   // sj is wave-uniform: indirect register addressing
                const float vo = vmV[sj], dq = dV[sj];
                vmV[sj] = own ? -INFINITY : vo;
                dV[sj] = own ? INFINITY : dq;
            } else {
#pragma unroll
                for (int sl = 0; sl < NC; sl++) {
                    const bool hit = own && (sl == sj);
                    VM(sl) = hit ? -INFINITY : VM(sl);
                    DR(sl) = hit ? INFINITY : DR(sl);
                }
            }
        }
        if (skip) {
#pragma unroll
            for (int m = 0; m < CH; m++) cm[m] = fmin_raw(fmin3_raw(DR(m * 4), DR(m * 4 + 1), DR(m * 4 + 2)), DR(m * 4 + 3));
            c_relax++;
            c_skipped++;
            continue;
        }
        const f32x2 hh = {h, h};
#pragma unroll
        for (int m = 0; m < CH; m++) {
            const f32x2 x01 = {x[m].x, x[m].y}, x23 = {x[m].z, x[m].w};
            const f32x2 v01 = {vmV[4 * m], vmV[4 * m + 1]}, v23 = {vmV[4 * m + 2], vmV[4 * m + 3]};
            const f32x2 a = (x01 - v01) - hh, b = (x23 - v23) - hh;
            dV[4 * m] = fmin_raw(dV[4 * m], a[0]);
            dV[4 * m + 1] = fmin_raw(dV[4 * m + 1], a[1]);
            dV[4 * m + 2] = fmin_raw(dV[4 * m + 2], b[0]);
            dV[4 * m + 3] = fmin_raw(dV[4 * m + 3], b[1]);
            cm[m] = fmin_raw(fmin3_raw(dV[4 * m], dV[4 * m + 1], dV[4 * m + 2]), dV[4 * m + 3]);
            SCHED_FENCE();
        }
        c_relax++;
    }
    // ---- the augmenting path, from the end column back to the free row (prices are still the search's prices) ----
    __syncthreads();   // the scan log and the retired columns' records are complete
    {
        int ep = endofpath;
        float dep = curmin;                                   // the end column's distance is the final minimum
        for (;;) {
            const float vep = st_vget<LDS_STATE>(s_v, gv, ep);
            // candidates in the oracle's order: entry 0 = the free row's initial scan (offset 0: fl(x - 0) = x), entry k + 1
            // = logged scan k.  Up to 8 gathers of c[row][ep] in flight per lane: one pass for <= 4095 scans.
            uint32_t first = 0xFFFFFFFFu;
            float cfirst = 0.0f;
            for (int e0 = 0; e0 <= nlog; e0 += 8 * BS) {
                float cv[8], hv[8];
#pragma unroll
                for (int t = 0; t < 8; t++) {
                    const int e = e0 + t * BS + tid;
                    const bool in = e >= 1 && e <= nlog;
                    const int row = in ? ld_i32(slog_row + e - 1) : freerow;
                    hv[t] = in ? ld_f32(slog_h + e - 1) : 0.0f;
                    cv[t] = cost[row_off(rowmap, row, ld) + ep];
                }
#pragma unroll
                for (int t = 7; t >= 0; t--) {
                    const int e = e0 + t * BS + tid;
                    if (e <= nlog && ((cv[t] - vep) - hv[t]) == dep) { first = umin32(first, (uint32_t)e); if (first == (uint32_t)e) cfirst = cv[t]; }
                }
                if (__syncthreads_or(first != 0xFFFFFFFFu)) break;   // a match in this pass precedes every later entry
            }
            const uint32_t f = wg_min_u32<NWV>(first, s, par);
            if (f == 0xFFFFFFFFu) return CYTO_ERR_INTERNAL;
            const int i = f == 0u ? freerow : __builtin_amdgcn_readfirstlane(ld_i32(slog_row + (int)f - 1));
            const int nxt = __builtin_amdgcn_readfirstlane(ld_i32(rowsol + i));
            __builtin_amdgcn_s_barrier();                     // every wave holds the old rowsol[i] before it is overwritten
            if (first == f) {                                 // the lane that evaluated the winning entry holds c[i][ep]
                st_csset<LDS_STATE>(s_cs, gcolsol, ep, i);
                if (LEAN || s_ca) l_ca[ep] = cfirst; else st_f32(cassign + ep, cfirst);
                if (gmode) { const int gi = rowgid[i]; if (LEAN || s_cg) l_cg[ep] = (uint16_t)gi; else st_i32(colgroup + ep, gi); }
                st_i32(rowsol + i, ep);
            }
            c_hops++;
            if (i == freerow) break;
            ep = nxt;
            dep = ld_f32(&sd[ep].y);                          // the distance this (scanned) column was retired at
        }
    }
    // price update: columns scanned at an earlier level than the final one.  (LDS prices: every lane updates its own
    // columns, nobody reads another lane's before the barrier below.)
#pragma unroll
    for (int sl = 0; sl < NC; sl++)
        if ((readym >> sl) & 1) st_vset<LDS_STATE>(s_v, gv, SLOT_COL(BS, sl), ld_f32(&sd[SLOT_COL(BS, sl)].x) - curmin);
    __syncthreads();
#undef VM
#undef DR
    return 0;
}

enum { PH_RT = 0, PH_ARR = 1, PH_AUG = 2 };

// CS_LDS (only meaningful with !LDS_STATE, n <= 65535): the prices are too many for LDS but colsol (u16) still fits;
// the chain then never stores colsol to global memory (on gfx9 a load is not returned before the stores issued
// ahead of it are acknowledged, so every global store in the step delays the next step's gathers).
template <int CH, bool LDS_STATE, bool CS_LDS = false>
__global__ __launch_bounds__(BLOCK2) void jv_chain2(const Chain2Args *__restrict__ batch) {
    const Chain2Args a = load_args(batch);       // one workgroup per problem of the batch
    constexpr int NC = CH * 4;
    constexpr bool CSL = LDS_STATE || CS_LDS;     // colsol lives in LDS
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    __shared__ Scratch2 s;
    __shared__ int32_t s_app[64];          // staged appends to the next sweep's free-row list (wave 0)
    const int tid = threadIdx.x, lane = tid & 63;
    // provably wave-uniform wave id: the wave-0 state machine below then lives in SGPRs with scalar branches
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = a.n;
    const int64_t ld = a.ld;
    const float *__restrict__ cost = a.cost;
    float *gv = a.fws;
    int32_t *rowsol = a.iws, *gcolsol = a.iws + n, *matches = a.iws + 2 * (int64_t)n;
    int32_t *freerows = a.iws + 3 * (int64_t)n, *rtrows = a.iws + 4 * (int64_t)n;
    const int npad = (n + 3) & ~3;
    float *s_v = reinterpret_cast<float *>(dyn_lds);
    uint16_t *s_cs = reinterpret_cast<uint16_t *>(dyn_lds + (LDS_STATE ? (size_t)npad * 4 : 0));
    int par = 0;

    uint64_t validm = 0;
#pragma unroll
    for (int sl = 0; sl < NC; sl++) if (SLOT_COL(BLOCK2, sl) < n) validm |= (1ull << sl);

    if constexpr (CSL) {
        for (int c = tid; c < npad; c += BLOCK2) {
            if constexpr (LDS_STATE) s_v[c] = c < n ? gv[c] : 0.0f;
            const int32_t cs = c < n ? gcolsol[c] : -1;
            s_cs[c] = cs < 0 ? (uint16_t)0xFFFFu : (uint16_t)cs;
        }
    }

    // ---- free-row list (matches == 0) and reduction-transfer list (matches == 1), ascending ----
    int numfree = 0, nrt = 0;
    {
        const int R = (n + BLOCK2 - 1) / BLOCK2;
        const int r0 = min(n, tid * R), r1 = min(n, r0 + R);
        int f = 0, g = 0;
        for (int i = r0; i < r1; i++) { const int mt = matches[i]; f += (mt == 0); g += (mt == 1); }
        int of = wg_exscan2(f, s, par, &numfree);
        int og = wg_exscan2(g, s, par, &nrt);
        for (int i = r0; i < r1; i++) {
            const int mt = matches[i];
            if (mt == 0) st_i32(freerows + of++, i);
            else if (mt == 1) st_i32(rtrows + og++, i);
        }
    }
    __syncthreads();

    float delta = 0.0f, tau_guess = INFINITY;
    int c_rt = 0, c_arr = 0, c_dense = 0;
    int c_free_cr = numfree, c_free_a1 = 0, c_free_a2 = 0;

    const int arr_budget = 1000 * n + 1000000;   // == JV_ARR_BUDGET(n) of the oracle (fits: n <= FAST_NMAX)
    // chain state (meaningful in wave 0 only; uniform there)
    int phase = (n > 1) ? PH_RT : PH_ARR;
    int k = 0, sweep = 0, prev = numfree, carry = -1, cur_i = -1;
    if (phase == PH_ARR) numfree = 0;
    bool have_dense = false;
    K2 gd; gd.m1 = KEYMAX; gd.m2 = KEYMAX;
    int napp = 0;                           // entries staged in s_app since the last flush

    for (;;) {
        if (wave == 0) {
            // wave 0 runs cached steps until it needs the whole workgroup (a dense re-scan) or is done;
            // it then posts a command and falls through to the barrier below.
            for (;;) {
                // ---------- slow path: choose the next row (phase changes, new chains, budget) ----------
                if (!have_dense) {
                    if (phase == PH_RT) {
                        if (k >= nrt) { phase = PH_ARR; sweep = 0; k = 0; prev = numfree; numfree = 0; carry = -1; continue; }
                        cur_i = __builtin_amdgcn_readfirstlane(ld_i32(rtrows + k)); k++;
                    } else if (phase == PH_ARR) {
                        if (c_arr >= arr_budget && (carry >= 0 || k < prev)) {
                            // step budget exhausted (see oracle/jv_oracle_impl.h): hand the waiting rows
                            // to the augmentation phase, the displaced row first, then the list order
                            if (lane < (napp & 63)) st_i32(freerows + numfree - (napp & 63) + lane, s_app[lane]);
                            napp = 0;
                            if (carry >= 0) { if (lane == 0) st_i32(freerows + numfree, carry); numfree++; carry = -1; }
                            while (k < prev) {
                                const int r = __builtin_amdgcn_readfirstlane(ld_i32(freerows + k)); k++;
                                if (lane == 0) st_i32(freerows + numfree, r);
                                numfree++;
                            }
                            continue;
                        }
                        if (carry >= 0) { cur_i = carry; carry = -1; }
                        else if (k < prev) { cur_i = __builtin_amdgcn_readfirstlane(ld_i32(freerows + k)); k++; }
                        else if (sweep == 0) {
                            if (lane < (napp & 63)) st_i32(freerows + numfree - (napp & 63) + lane, s_app[lane]);   // flush the staged tail
                            napp = 0;
                            c_free_a1 = numfree; sweep = 1; k = 0; prev = numfree; numfree = 0; continue;
                        }
                        else {
                            if (lane < (napp & 63)) st_i32(freerows + numfree - (napp & 63) + lane, s_app[lane]);
                            napp = 0;
                            c_free_a2 = numfree; phase = PH_AUG; k = 0; continue;
                        }
                    } else {
                        // RT and ARR are done: the augmentation runs in its own kernel (jv_aug2)
                        if (lane == 0) { s.cmd_op = OP_EXIT; s.cmd_row = 0; }
                        break;
                    }
                }
                if (phase == PH_RT) {
                    // v[j1] -= min over j != j1 of (c[i][j] - v[j])
                    const int i = cur_i;
                    const int j1 = __builtin_amdgcn_readfirstlane(ld_i32(rowsol + i));
                    float mn;
                    if (have_dense) {
                        have_dense = false;
                        mn = ((int)(uint32_t)gd.m1 == j1) ? key_val(gd.m2) : key_val(gd.m1);
                    } else {
                        const uint32_t col = ld_u32(a.cache_col + (int64_t)i * KC + lane);
                        const float cv = ld_f32(a.cache_val + (int64_t)i * KC + lane);
                        const float F = __uint_as_float(readlane32(__float_as_uint(cv), KCU));
                        const bool valid = col != COLSENT && (int)col != j1;
                        const float vj = st_vget<LDS_STATE>(s_v, gv, valid ? (int)col : 0);
                        mn = ord2f(wave_min_u32(valid ? f2ord(cv - vj) : 0xFFFFFFFFu));
                        if (!(mn < F)) {
                            if (lane == 0) { s.cmd_op = OP_REFRESH; s.cmd_row = i; }
                            c_dense++;
                            break;
                        }
                    }
                    const float nv = st_vget<LDS_STATE>(s_v, gv, j1) - mn;
                    if (lane == 0) st_vset<LDS_STATE>(s_v, gv, j1, nv);
                    c_rt++;
                    continue;
                }
                // ---------- ARR: tight loop that follows one displacement chain ----------
                // Software pipelining: the row that will be displaced (the next row of the chain) is known
                // right after the first reduction, so its cache is requested then and arrives while the second
                // reduction and the bookkeeping of the current step run.
                bool need_dense = false;
                int pf_row = -1;
                uint32_t pf_col = 0;
                float pf_cv = 0.0f;
                for (;;) {
                    const int i = cur_i;
                    float umin, usub, vj1, cj1 = 0.0f, cj2 = 0.0f;
                    int j1, j2 = -1, i0, i02 = -1;
                    if (__builtin_expect(have_dense, 0)) {
                        have_dense = false;
                        umin = key_val(gd.m1); usub = key_val(gd.m2);
                        j1 = (int)(uint32_t)gd.m1; j2 = (int)(uint32_t)gd.m2;
                        cj1 = a.cost[row_off(a.rowmap, i, a.ld) + j1]; cj2 = a.cost[row_off(a.rowmap, i, a.ld) + j2];
                        vj1 = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(st_vget<LDS_STATE>(s_v, gv, j1))));
                        i0 = __builtin_amdgcn_readfirstlane(st_csget<CSL>(s_cs, gcolsol, j1));
                        i02 = __builtin_amdgcn_readfirstlane(st_csget<CSL>(s_cs, gcolsol, j2));
                    } else {
                        uint32_t col;
                        float cv;
                        if (pf_row == i) { col = pf_col; cv = pf_cv; }          // requested during the previous step
                        else {
                            col = ld_u32(a.cache_col + (int64_t)i * KC + lane);
                            cv = ld_f32(a.cache_val + (int64_t)i * KC + lane);
                        }
                        const bool valid = col != COLSENT;
                        const float vj = st_vget<LDS_STATE>(s_v, gv, valid ? (int)col : 0);
                        const int32_t csj = st_csget<CSL>(s_cs, gcolsol, valid ? (int)col : 0);
                        const float F = __uint_as_float(readlane32(__float_as_uint(cv), KCU));
                        const uint32_t ord = valid ? f2ord(cv - vj) : 0xFFFFFFFFu;
                        // minimum, its lane (ties: lowest column), then the minimum of the rest
                        const uint32_t o1 = wave_min_u32(ord);
                        const uint64_t m1 = __ballot(ord == o1);
                        const int l1 = __builtin_ctzll(m1);     // cache rows are sorted by column: lowest lane = lowest column
                        // the current owner of the best column is (almost always) the next row of the chain
                        pf_row = (int)readlane32((uint32_t)csj, l1);
                        if (pf_row >= 0) {
                            pf_col = ld_u32(a.cache_col + (int64_t)pf_row * KC + lane);
                            pf_cv = ld_f32(a.cache_val + (int64_t)pf_row * KC + lane);
                        }
                        const uint32_t o2 = wave_min_u32(lane == l1 ? 0xFFFFFFFFu : ord);
                        usub = ord2f(o2);
                        if (__builtin_expect(!(usub < F), 0)) {
                            if (lane == 0) { s.cmd_op = OP_REFRESH; s.cmd_row = i; }
                            c_dense++;
                            need_dense = true;
                            break;
                        }
                        umin = ord2f(o1);
                        j1 = (int)readlane32(col, l1);
                        vj1 = __uint_as_float(readlane32(__float_as_uint(vj), l1));
                        cj1 = __uint_as_float(readlane32(__float_as_uint(cv), l1));
                        i0 = (int)readlane32((uint32_t)csj, l1);
                        if (__builtin_expect(!((vj1 - (usub - umin)) < vj1) && i0 >= 0, 0)) {
                            const uint64_t m2 = __ballot(ord == o2 && lane != l1);
                            const int l2 = __builtin_ctzll(m2);
                            j2 = (int)readlane32(col, l2);
                            cj2 = __uint_as_float(readlane32(__float_as_uint(cv), l2));
                            i02 = (int)readlane32((uint32_t)csj, l2);
                        }
                    }
                    c_arr++;
                    const float vnew = vj1 - (usub - umin);
                    const bool lowers = vnew < vj1;
                    const bool swap = !lowers && i0 >= 0;
                    const int jj = swap ? j2 : j1;
                    const int i0f = swap ? i02 : i0;
                    (void)cj1; (void)cj2;
                    // rowsol is not read during ARR and equals the inverse of colsol: it is rebuilt after the chain
                    if (lane == 0) {
                        if (lowers) st_vset<LDS_STATE>(s_v, gv, j1, vnew);
                        st_csset<CSL>(s_cs, gcolsol, jj, i);
                    }
                    if (__builtin_expect(i0f >= 0 && lowers && c_arr < arr_budget, 1)) { cur_i = i0f; continue; }   // chain goes on
                    if (i0f >= 0) {
                        if (lowers) carry = i0f;       // budget reached: the slow path flushes it
                        else {
                            // the next sweep's list is staged in LDS and written 64 entries at a time: a global store in
                            // every step would hold back the next step's loads until it is acknowledged
                            if (lane == 0) s_app[napp & 63] = i0f;
                            napp++; numfree++;
                            if ((napp & 63) == 0) st_i32(freerows + numfree - 64 + lane, s_app[lane]);
                        }
                    }
                    break;
                }
                if (need_dense) break;
            }
        }
        __syncthreads();
        const int op = s.cmd_op, row = s.cmd_row;
        if (op == OP_EXIT) break;
        if constexpr (CH == 0) {
            gd = refresh_row_stream<0x10>(row, n, ld, RBASE(cost, a.rowmap, row, ld), gv, a.cache_col, a.cache_val, delta, tau_guess, s, par);
            have_dense = true;
        } else {
            float vreg[NC > 0 ? NC : 1];
            load_vreg<CH, LDS_STATE>(s_v, gv, n, tid, vreg);
            gd = refresh_row<CH>(row, n, ld, RBASE(cost, a.rowmap, row, ld), vreg, validm, a.cache_col, a.cache_val, delta, s, par);
            have_dense = true;
        }
    }

    // ---- write back prices and colsol for the augmentation kernel; rowsol = inverse of colsol ----
    float *cassign = a.fws + 3 * (int64_t)n;
    int32_t *colgroup = a.iws + 6 * (int64_t)n;
    __syncthreads();
    for (int c = tid; c < n; c += BLOCK2) {
        const int32_t r = st_csget<CSL>(s_cs, gcolsol, c);
        if constexpr (LDS_STATE) gv[c] = s_v[c];
        if constexpr (CSL) gcolsol[c] = r;
        if (r >= 0) {
            rowsol[r] = c;
            cassign[c] = cost[row_off(a.rowmap, r, ld) + c];          // c[colsol[j]][j] for the augmentation kernel
            colgroup[c] = a.gmode ? a.rowgid[r] : 0;               // duplicate-row group of the row that owns column c
        }
    }
    if (tid == 0) {
        long long *counters = lap_status(a.misc)->counters;
        counters[C_RT] = c_rt; counters[C_ARR] = c_arr;
        counters[C_FREE_CR] = c_free_cr; counters[C_FREE_A1] = c_free_a1; counters[C_FREE_A2] = c_free_a2;
        counters[C2_DENSE_REFRESH] = c_dense;
        lap_status(a.misc)->numfree = numfree;
    }
}

// AUGMENTATION + duals + total: one persistent workgroup, all lanes active (see chain_augment).
// (BS is a parameter because a 256-thread variant -- one wave per SIMD, twice the columns per lane -- was measured: not faster,
// a lone wave per SIMD exposes the latency of every dependent instruction.)
template <int CH, bool LDS_STATE, int BS = BLOCK2>
__global__ __launch_bounds__(BS) void jv_aug2(const Chain2Args *__restrict__ batch) {
    const Chain2Args a = load_args(batch);       // one workgroup per problem of the batch
    constexpr int NC = CH * 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    __shared__ Scratch2 s;
    __shared__ PickRec s_rec[2][NW2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n;
    const int64_t ld = a.ld;
    const float *__restrict__ cost = a.cost;
    float *gv = a.fws;
    // per retired column (v + d, d) of the current search: the 2n floats behind cassign (jv_aug_lazy's distance words,
    // dead once this kernel runs); scan log: rows in the old predecessor slot, offsets in the old sumvd slot
    float2 *sd = reinterpret_cast<float2 *>(a.fws + 4 * (int64_t)n);
    float *slog_h = a.fws + 2 * (int64_t)n;
    int32_t *rowsol = a.iws, *gcolsol = a.iws + n;
    int32_t *freerows = a.iws + 3 * (int64_t)n, *slog_row = a.iws + 5 * (int64_t)n;
    const int npad = (n + 3) & ~3;
    float *s_v = reinterpret_cast<float *>(dyn_lds);
    uint16_t *s_cs = reinterpret_cast<uint16_t *>(dyn_lds + (size_t)npad * 4);
    int par = 0;
    uint64_t validm = 0;
#pragma unroll
    for (int sl = 0; sl < NC; sl++) if (SLOT_COL(BS, sl) < n) validm |= (1ull << sl);
    if constexpr (LDS_STATE) {
        for (int c = tid; c < npad; c += BS) {
            s_v[c] = c < n ? gv[c] : 0.0f;
            const int32_t cs = c < n ? gcolsol[c] : -1;
            s_cs[c] = cs < 0 ? (uint16_t)0xFFFFu : (uint16_t)cs;
        }
    }
    // per-group best offset of the current search (duplicate-row skip): LDS if it fits (gmode 1)
    float *hb = a.g_hbest;
    int32_t *hs = a.g_hstamp;
    const int gmode = a.gmode;
    if (gmode == 1) {
        hb = reinterpret_cast<float *>(dyn_lds + (size_t)npad * 6);
        hs = reinterpret_cast<int32_t *>(dyn_lds + (size_t)npad * 6 + (size_t)a.ngroups * 4);
        for (int g = tid; g < a.ngroups; g += BS) hs[g] = 0;
    }
    float *cassign = a.fws + 3 * (int64_t)n;
    // per-column auxiliaries (assigned cost, owner's row group) in LDS when they fit (a.auxlds)
    float *s_ca = nullptr;
    uint16_t *s_cg = nullptr;
    if (a.aug_start > 0 && gmode) {
        // continuing after jv_aug_lazy, which keeps no per-column group array: rebuild it from the assignment
        int32_t *colgroup = a.iws + 6 * (int64_t)n;
        for (int c = tid; c < n; c += BS) { const int32_t r = gcolsol[c]; colgroup[c] = r >= 0 ? a.rowgid[r] : 0; }
        __syncthreads();
    }
    if (a.auxlds) {
        const size_t off = (size_t)npad * 6 + (gmode == 1 ? (size_t)a.ngroups * 8 : 0);
        s_ca = reinterpret_cast<float *>(dyn_lds + ((off + 15) & ~(size_t)15));
        s_cg = reinterpret_cast<uint16_t *>(reinterpret_cast<unsigned char *>(s_ca) + (size_t)npad * 4);
        const int32_t *colgroup = a.iws + 6 * (int64_t)n;
        for (int c = tid; c < n; c += BS) { s_ca[c] = cassign[c]; s_cg[c] = (uint16_t)(gmode ? colgroup[c] : 0); }
    }
    __syncthreads();
    const int numfree = lap_status(a.misc)->numfree;
    long long c_relax = 0, c_hops = 0, c_augs = 0, c_skipped = 0;
    long long rows0 = 0, base0 = 0;
    if (a.aug_start > 0) {   // carry the counters of the searches jv_aug_lazy completed
        const long long *cn = lap_status(a.misc)->counters;
        c_relax = cn[C_AUG_RELAX]; c_hops = cn[C_HOPS]; c_augs = cn[C_AUGS]; c_skipped = cn[C2_AUG_SKIPPED];
        rows0 = cn[C_ROWS_READ]; base0 = c_augs + c_relax - c_skipped;
    }
    int err = 0;
    for (int f = a.aug_start; f < numfree && !err; f++) {
        const int freerow = __builtin_amdgcn_readfirstlane(ld_i32(freerows + f));
        if (LDS_STATE && a.auxlds && gmode != 2)
            err = chain_augment<CH, LDS_STATE, BS, true>(n, ld, cost, gv, sd, cassign, rowsol, gcolsol, slog_row, slog_h, s_v, s_cs, freerow, validm,
                                                         s, par, c_relax, c_hops, c_skipped, gmode, a.rowgid, a.iws + 6 * (int64_t)n, hb, hs, f + 1,
                                                         s_ca, s_cg, s_rec, a.rowmap);
        else
            err = chain_augment<CH, LDS_STATE, BS, false>(n, ld, cost, gv, sd, cassign, rowsol, gcolsol, slog_row, slog_h, s_v, s_cs, freerow, validm,
                                                          s, par, c_relax, c_hops, c_skipped, gmode, a.rowgid, a.iws + 6 * (int64_t)n, hb, hs, f + 1,
                                                          s_ca, s_cg, s_rec, a.rowmap);
        c_augs++;
    }
    // ---- write back prices and colsol, then duals u and the total ----
    if constexpr (LDS_STATE) {
        for (int c = tid; c < n; c += BS) {
            gv[c] = s_v[c];
            const uint16_t cs = s_cs[c];
            gcolsol[c] = cs == 0xFFFFu ? -1 : (int32_t)cs;
        }
    }
    __syncthreads();
    float *gu = a.fws + n;
    double part = 0.0;
    for (int i = tid; i < n; i += BS) {
        const int j = ld_i32(rowsol + i);
        const float cij = cost[row_off(a.rowmap, i, ld) + j];
        const float vj = ld_f32(gv + j);
        gu[i] = cij - vj;
        part += (double)cij;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) s.sum[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < BS / 64; w++) t += s.sum[w];
        lap_status(a.misc)->total = t;
        long long *counters = lap_status(a.misc)->counters;
        counters[C_AUG_INIT] = c_augs; counters[C_AUG_RELAX] = c_relax; counters[C_AUGS] = c_augs; counters[C_HOPS] = c_hops;
        counters[C_ROWS_READ] = a.aug_start > 0 ? rows0 + (c_augs + c_relax - c_skipped - base0)
                                                : counters[C2_DENSE_REFRESH] + c_augs + c_relax - c_skipped;
        counters[C2_AUG_SKIPPED] = c_skipped;
        lap_status(a.misc)->status = err;
    }
}

// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ld_u64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u64(uint64_t *p, uint64_t x) { __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------
// Cache-certified augmentation ("lazy" Dijkstra): the row caches also serve the augmentation.
//
// Prices never increase (RT/ARR lower them; the augmentation's update v += d - curmin has d < curmin;
// the one-ulp rounding exception is handled below), so a row's cache floor F_i stays a lower bound of the
// reduced cost of every column outside its cache.  Let T be the smallest distance of an unassigned column
// seen so far in this search: the search ends at a distance <= T, and a column whose distance is > T when
// the search ends is never scanned, so its d and pred are never observed.  A scan of row i with offset h
// changes a non-cached column j to fl(fl(c-v_j) - h) >= fl(F_i - h); if that bound is > T the scan is
// observably identical to relaxing the <= 63 cached columns only.  Strictness matters: an update equal to
// T could decide a tie between two unassigned columns.  Otherwise the whole workgroup scans the row.
//
// State: one 64-bit word per column in L2-resident global memory, (ordered d << 32) | step of the scan
// that set it (unsigned min == "strictly smaller d wins, the earlier scan on equal d", i.e. the oracle's
// `v2 < d` rule; pred is recovered as the row of that step); never written again once the column is scanned.  The pick
// structure is in LDS: for each block of 64 columns the smallest (d, assigned?, column) key.  A cached
// step runs on wave 0 alone: LDS min over the block keys, three independent loads (cache row, the picked
// column's block for its new minimum, c[i][jp]), <= 63 fire-and-forget 64-bit atomic mins + LDS mins.
// Columns whose price ROSE by rounding in a price update (possible only by an ulp when v+d crosses a
// binade) are kept in an exception list and relaxed explicitly in every cached step.
// ------------------------------------------------------------------------------------------
//   srow: [n+1]; dkey: [n] 64-bit distance words; rowgid / rowmap as in Chain2Args
//   may_bail   a dense kernel can take over: give up when the cache certificates keep failing
//   debug_exc  tests: pretend the first debug_exc columns had a price rounded upwards (exception list)
#define LAZY_FIELDS(P, S)                                                                                                \
    S(int, n) S(int64_t, ld) P(const float, cost) P(float, gv) P(float, gu) P(float, sumvd) P(float, cassign) P(uint64_t, dkey) \
    P(int32_t, rowsol) P(int32_t, colsol) P(int32_t, freerows) P(int32_t, srow) P(int32_t, slist) P(int32_t, slevel)          \
    P(const int32_t, rowgid) P(const int32_t, rowmap) P(const uint32_t, cache_col) P(const float, cache_val)                  \
    P(float, g_hbest) P(int32_t, g_hstamp) P(char, misc) S(int, ngroups) S(int, gmode) S(int, may_bail) S(int, debug_exc)
struct LazyArgs { LAZY_FIELDS(F_PTR, F_VAL) };
struct LazyArgsG { LAZY_FIELDS(F_GPTR, F_VAL) };
static_assert(sizeof(LazyArgs) == sizeof(LazyArgsG), "mirror layout");
__device__ __forceinline__ LazyArgs load_args(const LazyArgs *__restrict__ batch) {
    const LazyArgsG g = reinterpret_cast<const LazyArgsG *>(batch)[blockIdx.x];
    LazyArgs a;
    LAZY_FIELDS(F_COPY_PTR, F_COPY_VAL)
    return a;
}
struct LazyCmd { int op, row, step, stamp; float h; };
enum { LZ_DENSE = 1, LZ_EXIT = 2, LZ_ERR = 3, LZ_INIT_DENSE = 4 };
constexpr int LZ_MAXEXC = 64;

__device__ __forceinline__ void lds_min_u64(uint64_t *p, uint64_t x) {
    (void)__hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void gl_min_u64(uint64_t *p, uint64_t x) {
    (void)__hip_atomic_fetch_min(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr uint64_t LZ_INFKEY = 0xFFFFFFFF00000000ull;   // "no distance yet": any real d wins the unsigned min
// Before a column's word is used in this search its block of 64 words must hold this search's values:
// blocks are reset lazily (all 64 words = "no distance") the first time a search touches them.
__device__ __forceinline__ void lz_touch_blocks(bool act, int myblk, int myepoch, uint64_t *dkey, int32_t *s_ep, int32_t *s_tl,
                                                int &ntouch, int stamp, int npad, int lane) {
    uint64_t todo = __ballot(act && myepoch != stamp);
    while (todo) {
        const int l = __builtin_ctzll(todo);
        const int b = (int)readlane32((uint32_t)myblk, l);
        if (b * 64 + lane < npad) st_u64(dkey + b * 64 + lane, LZ_INFKEY);
        if (lane == 0) { s_ep[b] = stamp; s_tl[ntouch] = b; }
        ntouch++;
        todo &= ~__ballot(myblk == b);
    }
}
// LDS_STATE: prices and colsol in LDS; CS_LDS (with !LDS_STATE, n <= 65535): colsol (u16) in LDS, prices in L2
template <bool LDS_STATE, bool CS_LDS = false>
__global__ __launch_bounds__(BLOCK2) void jv_aug_lazy(const LazyArgs *__restrict__ batch) {
    const LazyArgs a = load_args(batch);         // one workgroup per problem of the batch
    constexpr bool CSL = LDS_STATE || CS_LDS;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    __shared__ Scratch2 s;
    __shared__ LazyCmd cmd;
    __shared__ int s_nexc;
    __shared__ uint32_t s_T;          // ordered key of T (wave 0 lowers it with LDS atomic mins)
    // the per-scan records of the current search (column, level, v + d, row) are staged here and written to the
    // global lists 64 at a time: every global store in a step holds back the next step's loads until it is acknowledged
    __shared__ int32_t s_ljp[64], s_llv[64], s_lrw[64];
    __shared__ float s_lsv[64];
    __shared__ int s_exc[LZ_MAXEXC];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = a.n;
    const int64_t ld = a.ld;
    const float *__restrict__ cost = a.cost;
    const int nquad = (n + 3) >> 2, npad = nquad * 4, nb = (n + 63) >> 6;
    float *gv = a.gv;
    size_t off = 0;
    float *s_v = nullptr;
    uint16_t *s_cs = nullptr;
    if constexpr (LDS_STATE) {
        s_v = reinterpret_cast<float *>(dyn_lds);
        s_cs = reinterpret_cast<uint16_t *>(dyn_lds + (size_t)npad * 4);
        off = ((size_t)npad * 6 + 15) & ~(size_t)15;
    } else if constexpr (CS_LDS) {
        s_cs = reinterpret_cast<uint16_t *>(dyn_lds);
        off = ((size_t)npad * 2 + 15) & ~(size_t)15;
    }
    const int nbp = (nb + 511) & ~511;               // padded with KEYMAX: the pick reads 8 keys per lane, unpredicated
    uint64_t *bmin = reinterpret_cast<uint64_t *>(dyn_lds + off); off += (size_t)nbp * 8;
    uint32_t *s_sc = reinterpret_cast<uint32_t *>(dyn_lds + off); off += (size_t)nb * 8;   // 2 words per block
    uint32_t *s_un = reinterpret_cast<uint32_t *>(dyn_lds + off); off += (size_t)nb * 8;
    int32_t *s_ep = reinterpret_cast<int32_t *>(dyn_lds + off); off += (size_t)nb * 4;   // search stamp of each block's dkey words
    int32_t *s_tl = reinterpret_cast<int32_t *>(dyn_lds + off); off += (size_t)nb * 4;   // blocks touched by the current search
    off = (off + 7) & ~(size_t)7;
    const int gmode = a.gmode;
    float *hb = a.g_hbest;
    int32_t *hs = a.g_hstamp;
    if (gmode == 1) {
        hb = reinterpret_cast<float *>(dyn_lds + off);
        hs = reinterpret_cast<int32_t *>(dyn_lds + off + (size_t)a.ngroups * 4);
        for (int g = tid; g < a.ngroups; g += BLOCK2) hs[g] = 0;
    }
    int par = 0;
    if constexpr (CSL) {
        for (int c = tid; c < npad; c += BLOCK2) {
            if constexpr (LDS_STATE) s_v[c] = c < n ? gv[c] : 0.0f;
            const int32_t cs = c < n ? a.colsol[c] : -1;
            s_cs[c] = cs < 0 ? (uint16_t)0xFFFFu : (uint16_t)cs;
        }
    }
    for (int w = tid; w < 2 * nb; w += BLOCK2) {
        uint32_t m = 0;
        for (int b = 0; b < 32; b++) { const int c = w * 32 + b; if (c < n && a.colsol[c] < 0) m |= (1u << b); }
        s_un[w] = m;
    }
    if (tid == 0) s_nexc = a.debug_exc;
    if (tid < LZ_MAXEXC) s_exc[tid] = tid < n ? tid : 0;
    for (int b = tid; b < nb; b += BLOCK2) s_ep[b] = 0;
    long long c_sparse = 0;
    // between searches: every block minimum is "empty", no column is marked scanned
    for (int b = tid; b < nbp; b += BLOCK2) bmin[b] = KEYMAX;
    for (int w = tid; w < 2 * nb; w += BLOCK2) s_sc[w] = 0;
    __syncthreads();
    const int numfree = lap_status(a.misc)->numfree;
    long long c_relax = 0, c_hops = 0, c_augs = 0, c_skipped = 0, c_dense = 0;
    int err = 0;
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(gv, 0, nquad * 16, 0x00020000);
    const __amdgpu_buffer_rsrc_t rdk = __builtin_amdgcn_make_buffer_rsrc(a.dkey, 0, nquad * 32, 0x00020000);

    // Wave 0 owns the control flow: it runs whole searches (sparse init, cached steps, price update, path flip)
    // on its own and calls the other waves in -- through `cmd` and the barrier below -- only for an operation
    // that needs a full cost row (dense init of a search, dense scan of a row).
    int f = 0, freerow = -1, stamp = 0;
    bool insearch = false, have = false, dense_used = false, isparse = false;
    float curmin = 0.0f, icv = 0.0f;
    uint32_t icc = COLSENT;
    int level = 0, nscan = 0, ntouch = 0;
    int nexc = a.debug_exc > LZ_MAXEXC ? LZ_MAXEXC : a.debug_exc;   // register copy of s_nexc (it only changes at a search's end)
    bool bail = false, no_cert = a.debug_exc > LZ_MAXEXC;
    long long w_relax0 = 0, w_dense0 = 0;           // start of the current hand-over window
    // software pipeline over searches: id of the free row after next, cache row of the next one
    int id_next = -1, id1_saved = -1;
    uint32_t ncc = COLSENT;
    float ncv = 0.0f;
    if (wave == 0 && numfree > 0) {
        const int id0 = __builtin_amdgcn_readfirstlane(ld_i32(a.freerows));
        ncc = ld_u32(a.cache_col + (int64_t)id0 * KC + lane);
        ncv = ld_f32(a.cache_val + (int64_t)id0 * KC + lane);
        id_next = numfree > 1 ? ld_i32(a.freerows + 1) : -1;
        freerow = id0;
    }
    for (;;) {
        if (wave == 0) {
            bool post = false;
            while (!post) {
                if (!insearch) {
                    if (f >= numfree || err || bail) { if (lane == 0) cmd.op = err ? LZ_ERR : LZ_EXIT; break; }
                    // (freerow, ncc, ncv) were requested during the previous search; request the next ones now
                    const uint32_t cc = ncc;
                    const float cv = ncv;
                    const int id1 = __builtin_amdgcn_readfirstlane(id_next);
                    id1_saved = id1;
                    stamp = f + 1;
                    have = false; curmin = 0.0f; level = 0; nscan = 0; ntouch = 0; dense_used = false; insearch = true;
                    // ---- certified sparse init: if the free row's cache floor is above the distance of an
                    // unassigned cached column, no column outside the cache can matter in this search ----
                    const bool valid = lane < KCU && cc != COLSENT;
                    const int j = valid ? (int)cc : 0;
                    const float dd = cv - st_vget<LDS_STATE>(s_v, gv, j);
                    const bool un = valid && ((s_un[j >> 5] >> (j & 31)) & 1u);
                    const uint32_t odd = valid ? f2ord(dd) : 0xFFFFFFFFu;
                    const uint32_t t0 = wave_min_u32(un ? odd : 0xFFFFFFFFu);
                    // only now the requests for the next search (loads return in issue order: issued before the price gather
                    // above, these cache-row loads from HBM would have held it back)
                    if (id1 >= 0) {
                        ncc = ld_u32(a.cache_col + (int64_t)id1 * KC + lane);
                        ncv = ld_f32(a.cache_val + (int64_t)id1 * KC + lane);
                    }
                    id_next = f + 2 < numfree ? ld_i32(a.freerows + f + 2) : -1;
                    const float floor_f = __uint_as_float(readlane32(__float_as_uint(cv), KCU));
                    const bool cert0 = !no_cert && nexc == 0 && t0 != 0xFFFFFFFFu && floor_f > ord2f(t0);
                    if (cert0 && wave_min_u32(odd) == t0) {
                        // ---- single-edge search: the smallest distance of the whole row belongs to an unassigned
                        // column (the oracle's first pick ends the search at once: no scan, no price update);
                        // nothing of the pick structure is touched ----
                        const uint64_t me = __ballot(un && odd == t0);
                        const int le = __builtin_ctzll(me);   // (cache rows are sorted by column: lowest lane = lowest column)
                        const int ep = (int)readlane32(cc, le);
                        const float cie = __uint_as_float(readlane32(__float_as_uint(cv), le));
                        if (lane == 0) {
                            st_csset<CSL>(s_cs, a.colsol, ep, freerow);
                            st_f32(a.cassign + ep, cie);
                            st_i32(a.rowsol + freerow, ep);
                            s_un[ep >> 5] &= ~(1u << (ep & 31));
                        }
                        c_hops++; c_augs++; c_sparse++;
                        f++;
                        freerow = id1_saved;
                        insearch = false;
                        continue;
                    }
                    if (cert0) {
                        const bool act = valid && !(dd > ord2f(t0));
                        lz_touch_blocks(act, j >> 6, s_ep[j >> 6], a.dkey, s_ep, s_tl, ntouch, stamp, npad, lane);
                        if (act) {
                            const uint32_t od = f2ord(dd);
                            st_u64(a.dkey + j, (uint64_t)od << 32);                 // step 0 = the free row
                            lds_min_u64(bmin + (j >> 6), ((uint64_t)od << 32) | (un ? 0u : 0x80000000u) | (uint32_t)j);
                        }
                        if (lane == 0) { s_T = t0; st_i32(a.srow, freerow); }
                        c_sparse++;
                        isparse = true; icc = cc; icv = cv;
                    } else {
                        if (lane == 0) { cmd.op = LZ_INIT_DENSE; cmd.row = freerow; cmd.stamp = stamp; }
                        isparse = false; dense_used = true; post = true;
                        continue;
                    }
                }
                for (;;) {
                    // ---- pick: smallest (d, assigned?, column) over the block minima ----
                    uint64_t k = KEYMAX;
                    for (int b0 = 0; b0 < nbp; b0 += 512) {
                        uint64_t kk[8];
#pragma unroll
                        for (int u = 0; u < 8; u++) kk[u] = bmin[b0 + u * 64 + lane];
#pragma unroll
                        for (int u = 0; u < 8; u++) k = umin64(k, kk[u]);
                    }
                    {   // value first; the low word only needs a second reduction when several lanes tie on d
                        const uint32_t hi = (uint32_t)(k >> 32);
                        const uint32_t m = wave_min_u32(hi);
                        const uint64_t eq = __ballot(hi == m);
                        uint32_t lo;
                        if (__builtin_popcountll(eq) == 1) lo = readlane32((uint32_t)k, __builtin_ctzll(eq));
                        else lo = wave_min_u32(hi == m ? (uint32_t)k : 0xFFFFFFFFu);
                        k = ((uint64_t)m << 32) | lo;
                    }
                    const float dmin = key_val(k);
                    if (k == KEYMAX || !(dmin < INFINITY)) { err = CYTO_ERR_INTERNAL; insearch = false; break; }
                    const int jp = (int)((uint32_t)k & 0x7FFFFFFFu);
                    if (!have || dmin != curmin) { level++; curmin = dmin; have = true; }
                    if (!((uint32_t)k & 0x80000000u)) {
                        // ======== end of the search (wave 0 alone): price update, path flip, clean-up ========
                        const int endofpath = jp;
                        {
                            const int rem = nscan & 63, base = nscan - rem;
                            if (lane < rem) {
                                st_i32(a.slist + base + lane, s_ljp[lane]); st_i32(a.slevel + base + lane, s_llv[lane]);
                                st_f32(a.sumvd + base + lane, s_lsv[lane]); st_i32(a.srow + 1 + base + lane, s_lrw[lane]);
                            }
                        }
                        for (int k2 = lane; k2 < nscan; k2 += 64) {
                            if (ld_i32(a.slevel + k2) < level) {
                                const int j = ld_i32(a.slist + k2);
                                const float vold = st_vget<LDS_STATE>(s_v, gv, j);
                                const float vnew = ld_f32(a.sumvd + k2) - curmin;
                                st_vset<LDS_STATE>(s_v, gv, j, vnew);
                                if (vnew > vold) {   // rounding pushed a price UP: column j leaves the cache certificates
                                    const int e = atomicAdd(&s_nexc, 1);
                                    if (e < LZ_MAXEXC) s_exc[e] = j;
                                }
                            }
                        }
                        nexc = s_nexc;
                        // more such columns than the list holds: the certificates are abandoned for the rest of the solve
                        // (every scan reads its full row; still exact, just slow) -- or the dense kernel takes over
                        if (nexc > LZ_MAXEXC) { nexc = LZ_MAXEXC; no_cert = true; if (a.may_bail) bail = true; }
                        // c[freerow][endofpath] is in the sparse init's cache row when the path is a single edge
                        float cie0 = 0.0f;
                        bool have_cie0 = false;
                        if (nscan == 0 && isparse) {
                            const uint64_t mm = __ballot(lane < KCU && icc == (uint32_t)endofpath);
                            if (mm) { cie0 = __uint_as_float(readlane32(__float_as_uint(icv), __builtin_ctzll(mm))); have_cie0 = true; }
                        }
                        int hops = 0;
                        if (lane == 0) {
                            int ep = endofpath;
                            const int st0 = nscan == 0 ? 0 : (int32_t)(uint32_t)ld_u64(a.dkey + ep);
                            int i = st0 == 0 ? freerow : ld_i32(a.srow + st0);
                            for (;;) {
                                st_csset<CSL>(s_cs, a.colsol, ep, i);
                                st_f32(a.cassign + ep, (have_cie0 && hops == 0) ? cie0 : cost[row_off(a.rowmap, i, ld) + ep]);
                                const int j1 = ep;
                                if (i != freerow) ep = ld_i32(a.rowsol + i);      // (the free row owns no column)
                                st_i32(a.rowsol + i, j1);
                                hops++;
                                if (i == freerow) break;
                                const int stp = (int32_t)(uint32_t)ld_u64(a.dkey + ep);
                                i = stp == 0 ? freerow : ld_i32(a.srow + stp);
                            }
                            s_un[endofpath >> 5] &= ~(1u << (endofpath & 31));
                        }
                        c_hops += __builtin_amdgcn_readfirstlane(hops);
                        // back to the between-searches state of the LDS pick structure
                        if (!dense_used) {
                            for (int k2 = lane; k2 < ntouch; k2 += 64) { const int b = s_tl[k2]; bmin[b] = KEYMAX; s_sc[2 * b] = 0; s_sc[2 * b + 1] = 0; }
                        } else {
                            for (int b = lane; b < nb; b += 64) { bmin[b] = KEYMAX; s_sc[2 * b] = 0; s_sc[2 * b + 1] = 0; }
                        }
                        c_augs++;
                        f++;
                        freerow = id1_saved;
                        insearch = false;
                        // instances whose searches run deeper than the caches reach (>= 10 % full-row scans) are
                        // faster on the register-resident dense kernel: hand the remaining free rows over
                        // (judged on windows of >= 8192 scans, so that a dense-heavy start alone does not decide)
                        if (a.may_bail && c_relax - w_relax0 >= 8192) {
                            if ((c_dense - w_dense0) * 10 >= c_relax - w_relax0) bail = true;
                            w_relax0 = c_relax; w_dense0 = c_dense;
                        }
                        break;
                    }
                    const int i = __builtin_amdgcn_readfirstlane(st_csget<CSL>(s_cs, a.colsol, jp));
                    const float vjp = st_vget<LDS_STATE>(s_v, gv, jp);
                    const int step = nscan + 1;
                    const int blk = jp >> 6;
                    const int jb = blk * 64 + lane;
                    // independent loads: c[i][jp], the row's cache, the picked column's block, the row's group
                    // (the cache row last: a skipped scan continues without waiting for it)
                    const float cip_raw = ld_f32(a.cassign + jp);
                    const uint64_t dk = jb < n ? ld_u64(a.dkey + jb) : 0ull;
                    const int g_raw = gmode ? a.rowgid[i] : 0;
                    const uint32_t cc = ld_u32(a.cache_col + (int64_t)i * KC + lane);
                    const float cv = ld_f32(a.cache_val + (int64_t)i * KC + lane);
                    // retire column jp
                    if (lane == 0) {
                        s_ljp[nscan & 63] = jp; s_llv[nscan & 63] = level; s_lsv[nscan & 63] = vjp + dmin; s_lrw[nscan & 63] = i;
                        atomicOr(&s_sc[jp >> 5], 1u << (jp & 31));
                    }
                    const uint32_t scw = s_sc[blk * 2 + (lane >> 5)], unw = s_un[blk * 2 + (lane >> 5)];
                    const float cip = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(cip_raw)));
                    const float h = (cip - vjp) - curmin;
                    // (the word of a scanned column is never written again -- every writer tests the scanned bit -- so it
                    // keeps the step that set its distance: that is its predecessor for the path flip)
                    bool skip = false;
                    if (gmode) {
                        const int g = __builtin_amdgcn_readfirstlane(g_raw);
                        float hbv; int hsv;
                        if (gmode == 1) { hbv = hb[g]; hsv = hs[g]; } else { hbv = ld_f32(hb + g); hsv = ld_i32(hs + g); }
                        skip = (hsv == stamp) && (h <= hbv);
                        if (!skip && lane == 0) {
                            if (gmode == 1) { hb[g] = h; hs[g] = stamp; } else { st_f32(hb + g, h); st_i32(hs + g, stamp); }
                        }
                    }
                    // new minimum of the picked column's block (this step's relaxations are applied after it)
                    {
                        const bool live = jb < n && !((scw >> (lane & 31)) & 1u);
                        const bool unb = (unw >> (lane & 31)) & 1u;
                        const uint32_t hi = live ? (uint32_t)(dk >> 32) : 0xFFFFFFFFu;
                        const uint32_t m = wave_min_u32(hi);
                        const uint64_t eq = __ballot(live && hi == m), equ = __ballot(live && hi == m && unb);
                        uint64_t kb = KEYMAX;
                        if (eq) {   // lane order is column order inside a block: lowest unassigned lane, else lowest lane
                            const int wl = equ ? __builtin_ctzll(equ) : __builtin_ctzll(eq);
                            kb = ((uint64_t)m << 32) | (equ ? 0u : 0x80000000u) | (uint32_t)(blk * 64 + wl);
                        }
                        if (lane == 0) bmin[blk] = kb;
                    }
                    nscan++;
                    c_relax++;
                    if ((nscan & 63) == 0) {
                        const int base = nscan - 64;
                        st_i32(a.slist + base + lane, s_ljp[lane]); st_i32(a.slevel + base + lane, s_llv[lane]);
                        st_f32(a.sumvd + base + lane, s_lsv[lane]); st_i32(a.srow + 1 + base + lane, s_lrw[lane]);
                    }
                    if (skip) { c_skipped++; continue; }
                    const float floor_i = __uint_as_float(readlane32(__float_as_uint(cv), KCU));
                    const float T = ord2f(s_T);
                    if (no_cert || !((floor_i - h) > T)) {
                        if (lane == 0) { cmd.op = LZ_DENSE; cmd.row = i; cmd.step = step; cmd.h = h; cmd.stamp = stamp; }
                        dense_used = true; post = true;
                        break;
                    }
                    // ---- cached relaxation: lane = cache entry; plus the (normally empty) exception list ----
                    {
                        const bool valid = lane < KCU && cc != COLSENT;
                        const int j = valid ? (int)cc : 0;
                        // one round of LDS gathers: price, scanned / unassigned words, the block's search stamp
                        const float vj = st_vget<LDS_STATE>(s_v, gv, j);
                        const uint32_t scw = s_sc[j >> 5], unw = s_un[j >> 5];
                        const int32_t epj = s_ep[j >> 6];
                        const float v2 = (cv - vj) - h;
                        const bool scn = (scw >> (j & 31)) & 1u;
                        const bool act = valid && !scn && !(v2 > T);
                        lz_touch_blocks(act, j >> 6, epj, a.dkey, s_ep, s_tl, ntouch, stamp, npad, lane);
                        if (act) {
                            const bool un = (unw >> (j & 31)) & 1u;
                            const uint32_t o2 = f2ord(v2);
                            gl_min_u64(a.dkey + j, ((uint64_t)o2 << 32) | (uint32_t)step);
                            lds_min_u64(bmin + (j >> 6), ((uint64_t)o2 << 32) | (un ? 0u : 0x80000000u) | (uint32_t)j);
                            if (un) atomicMin(&s_T, o2);
                        }
                    }
                    if (nexc > 0) {
                        const bool ev = lane < nexc;
                        const int j = ev ? s_exc[lane] : 0;
                        const float vj = st_vget<LDS_STATE>(s_v, gv, j);
                        const float v2 = ev ? (cost[row_off(a.rowmap, i, ld) + j] - vj) - h : 0.0f;
                        const bool scn = (s_sc[j >> 5] >> (j & 31)) & 1u;
                        lz_touch_blocks(ev && !scn, j >> 6, s_ep[j >> 6], a.dkey, s_ep, s_tl, ntouch, stamp, npad, lane);
                        if (ev && !scn) {
                            const bool un = (s_un[j >> 5] >> (j & 31)) & 1u;
                            const uint32_t o2 = f2ord(v2);
                            gl_min_u64(a.dkey + j, ((uint64_t)o2 << 32) | (uint32_t)step);
                            lds_min_u64(bmin + (j >> 6), ((uint64_t)o2 << 32) | (un ? 0u : 0x80000000u) | (uint32_t)j);
                            if (un) atomicMin(&s_T, o2);
                        }
                    }
                }
            }
        }
        __syncthreads();                               // command posted; wave 0's global traffic drained
        {
            const int op = cmd.op;
            if (op == LZ_ERR) { err = CYTO_ERR_INTERNAL; break; }
            if (op == LZ_EXIT) break;
            const int stamp = cmd.stamp;               // (shadows wave 0's copy with the same value)
            if (op == LZ_INIT_DENSE) {
                const int freerow = cmd.row;
                // ================= dense init: d = c[freerow] - v for every column (whole workgroup) =================
                        float tl = INFINITY;
                {
                    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<float *>(cost + row_off(a.rowmap, freerow, ld)), 0, (int)(ld * 4), 0x00020000);
                    for (int q0 = 0; q0 < nquad; q0 += BLOCK2) {
                        const int q = q0 + tid;
                        uint64_t bk = KEYMAX;
                        if (q < nquad) {
                            const u32x4_t xr = __builtin_amdgcn_raw_buffer_load_b128(rr, q * 16, 0, 0);
                            float4 vv;
                            if constexpr (LDS_STATE) vv = *reinterpret_cast<const float4 *>(s_v + q * 4);
                            else {
                                const u32x4_t vr = __builtin_amdgcn_raw_buffer_load_b128(rv, q * 16, 0, 0x10);
                                vv = make_float4(__uint_as_float(vr.x), __uint_as_float(vr.y), __uint_as_float(vr.z), __uint_as_float(vr.w));
                            }
                            const uint32_t um = (s_un[q >> 3] >> ((q & 7) * 4)) & 0xFu;
                            const float xs[4] = {__uint_as_float(xr.x), __uint_as_float(xr.y), __uint_as_float(xr.z), __uint_as_float(xr.w)};
                            const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
                            uint64_t dq[4] = {0, 0, 0, 0};
        #pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int c = q * 4 + e;
                                if (c < n) {
                                    const float dd = xs[e] - vs[e];
                                    const uint32_t od = f2ord(dd);
                                    const bool un = (um >> e) & 1u;
                                    dq[e] = (uint64_t)od << 32;                       // step 0 = the free row
                                    bk = umin64(bk, ((uint64_t)od << 32) | (un ? 0u : 0x80000000u) | (uint32_t)c);
                                    if (un) tl = fminf(tl, dd);
                                }
                            }
                            // dkey has npad entries: whole quads are stored (the pad words are never read)
                            const u32x4_t w0 = {(uint32_t)dq[0], (uint32_t)(dq[0] >> 32), (uint32_t)dq[1], (uint32_t)(dq[1] >> 32)};
                            const u32x4_t w1 = {(uint32_t)dq[2], (uint32_t)(dq[2] >> 32), (uint32_t)dq[3], (uint32_t)(dq[3] >> 32)};
                            __builtin_amdgcn_raw_buffer_store_b128(w0, rdk, q * 32, 0, 0x10);
                            __builtin_amdgcn_raw_buffer_store_b128(w1, rdk, q * 32 + 16, 0, 0x10);
                        }
                        bk = min64_row_allreduce(bk);          // 16 lanes = 16 quads = one block of 64 columns
                        if ((lane & 15) == 0 && q < nquad) { bmin[q >> 4] = bk; s_ep[q >> 4] = stamp; }
                    }
                }
                if (tid == 0) st_i32(a.srow, freerow);
                {
                    const uint32_t t0 = wg_min_u32(f2ord(tl), s, par);
                    if (tid == 0) s_T = t0;
                }
                __syncthreads();
                continue;
            }
            // ================= dense scan of row cmd.row (certificate failed): whole workgroup =================
            // Only a relaxation to a value <= T (the threshold when the scan starts; T only decreases) can be observed,
            // so the per-column words are touched for those columns only; a 64-column block none of whose columns
            // matters is skipped altogether, one that is met for the first time in this search is initialised here.
            {
                const int i = cmd.row, step = cmd.step;
                const float h = cmd.h;
                const float T0 = ord2f(s_T);
                const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float *>(cost + row_off(a.rowmap, i, ld)), 0, (int)(ld * 4), 0x00020000);
                float tl2 = INFINITY;
                for (int q0 = 0; q0 < nquad; q0 += BLOCK2) {
                    const int q = q0 + tid;
                    uint32_t o2s[4] = {0, 0, 0, 0};
                    uint32_t okm = 0, um = 0;
                    if (q < nquad) {
                        const u32x4_t xr = __builtin_amdgcn_raw_buffer_load_b128(rr, q * 16, 0, 0);
                        float4 vv;
                        if constexpr (LDS_STATE) vv = *reinterpret_cast<const float4 *>(s_v + q * 4);
                        else {
                            const u32x4_t vr = __builtin_amdgcn_raw_buffer_load_b128(rv, q * 16, 0, 0x10);
                            vv = make_float4(__uint_as_float(vr.x), __uint_as_float(vr.y), __uint_as_float(vr.z), __uint_as_float(vr.w));
                        }
                        um = (s_un[q >> 3] >> ((q & 7) * 4)) & 0xFu;
                        const uint32_t sm = (s_sc[q >> 3] >> ((q & 7) * 4)) & 0xFu;
                        const float xs[4] = {__uint_as_float(xr.x), __uint_as_float(xr.y), __uint_as_float(xr.z), __uint_as_float(xr.w)};
                        const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int c = q * 4 + e;
                            const float v2 = (xs[e] - vs[e]) - h;
                            o2s[e] = f2ord(v2);
                            if (c < n && !((sm >> e) & 1u) && !(v2 > T0)) {
                                okm |= 1u << e;
                                if ((um >> e) & 1u) tl2 = fminf(tl2, v2);
                            }
                        }
                    }
                    // does any column of my block (16 lanes = 64 columns) matter?
                    const uint64_t hitm = __ballot(okm != 0);
                    if ((hitm >> (lane & 48)) & 0xFFFFull) {
                        const int b = q >> 4;
                        const bool fresh = q < nquad && s_ep[b] == stamp;
                        const bool first = q < nquad && !fresh;
                        uint64_t bk = KEYMAX;
                        if (fresh) {
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                if ((okm >> e) & 1u) {
                                    const int c = q * 4 + e;
                                    const uint64_t dkc = ld_u64(a.dkey + c);
                                    if (o2s[e] < (uint32_t)(dkc >> 32)) {
                                        st_u64(a.dkey + c, ((uint64_t)o2s[e] << 32) | (uint32_t)step);
                                        bk = umin64(bk, ((uint64_t)o2s[e] << 32) | (((um >> e) & 1u) ? 0u : 0x80000000u) | (uint32_t)c);
                                    }
                                }
                            }
                        } else if (first) {
                            uint64_t dq[4];
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int c = q * 4 + e;
                                dq[e] = LZ_INFKEY;
                                if ((okm >> e) & 1u) {
                                    dq[e] = ((uint64_t)o2s[e] << 32) | (uint32_t)step;
                                    bk = umin64(bk, ((uint64_t)o2s[e] << 32) | (((um >> e) & 1u) ? 0u : 0x80000000u) | (uint32_t)c);
                                }
                            }
                            const u32x4_t w0 = {(uint32_t)dq[0], (uint32_t)(dq[0] >> 32), (uint32_t)dq[1], (uint32_t)(dq[1] >> 32)};
                            const u32x4_t w1 = {(uint32_t)dq[2], (uint32_t)(dq[2] >> 32), (uint32_t)dq[3], (uint32_t)(dq[3] >> 32)};
                            __builtin_amdgcn_raw_buffer_store_b128(w0, rdk, q * 32, 0, 0x10);
                            __builtin_amdgcn_raw_buffer_store_b128(w1, rdk, q * 32 + 16, 0, 0x10);
                        }
                        bk = min64_row_allreduce(bk);
                        if ((lane & 15) == 0 && q < nquad) {
                            if (bk != KEYMAX) lds_min_u64(bmin + b, bk);
                            s_ep[b] = stamp;
                        }
                    }
                }
                {
                    const uint32_t t2 = wg_min_u32(f2ord(tl2), s, par);
                    if (tid == 0) atomicMin(&s_T, t2);
                }
                c_dense++;
                __syncthreads();
            }
        }
    }
    // ---- write back prices and colsol, then duals u and the total ----
    if constexpr (CSL) {
        for (int c = tid; c < n; c += BLOCK2) {
            if constexpr (LDS_STATE) gv[c] = s_v[c];
            const uint16_t cs = s_cs[c];
            a.colsol[c] = cs == 0xFFFFu ? -1 : (int32_t)cs;
        }
    }
    __syncthreads();
    double part = 0.0;
    for (int i = tid; i < n; i += BLOCK2) {
        const int j = ld_i32(a.rowsol + i);
        if (j < 0) continue;              // still free: the kernel gave up and the dense kernel finishes (and redoes this)
        const float cij = cost[row_off(a.rowmap, i, ld) + j];
        const float vj = ld_f32(gv + j);
        a.gu[i] = cij - vj;
        part += (double)cij;
    }
#pragma unroll
    for (int off2 = 32; off2 >= 1; off2 >>= 1) part += __shfl_xor(part, off2);
    if (lane == 0) s.sum[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < NW2; w++) t += s.sum[w];
        lap_status(a.misc)->total = t;
        long long *counters = lap_status(a.misc)->counters;
        counters[C_AUG_INIT] = c_augs; counters[C_AUG_RELAX] = c_relax; counters[C_AUGS] = c_augs; counters[C_HOPS] = c_hops;
        counters[C_ROWS_READ] = counters[C2_DENSE_REFRESH] + (c_augs - c_sparse) + c_dense;
        counters[C2_AUG_SKIPPED] = c_skipped;
        counters[C2_AUG_DENSE] = c_dense;
        counters[C2_AUG_SPARSE_INIT] = c_sparse;
        lap_status(a.misc)->lazy_done = f;
        lap_status(a.misc)->status = err;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

enum { ST_GHB = 0, ST_GHS, ST_LZHB, ST_LZHS };     // SolveJob::state[]: per-group best offsets and stamps of jv_chain2 / jv_aug2, of jv_aug_lazy
static_assert(ST_LZHS + 1 == CHAIN_STATE_BUFS, "the caller's buffers");

// prices and colsol of the chain in LDS: by size, unless a large-n variant is forced at a small n (cyto_lap_opts.chain_variant; the
// test-suite runs them on instances the CPU oracle solves in a second)
static bool chain_lds_variant(const ChainPlan &pl) { return pl.variant == 0 && pl.n <= 13 * 4 * BLOCK2; }
// cache-certified augmentation: the default above 5120 columns (measured cross-over with the register-resident dense
// search on uniform and duplicated-row instances), the only one beyond 26 624
static bool chain_lazy(const ChainPlan &pl) {
    return pl.augmentation == 2 || !chain_lds_variant(pl) || (pl.augmentation == 0 && pl.n > 5120);
}

struct ChainLaunch {            // what chain_solve_batch has worked out for the launches of the batch
    bool lazy, lz_lds_state, lz_cs_lds, no_cs_lds;
    size_t shm_chain, shm_aug = 0, shm_lazy = 0;        // dynamic LDS of jv_chain2, jv_aug2, jv_aug_lazy (the most a problem of the batch asks for)
    std::vector<Chain2Args> c2;                         // argument blocks, a problem each
    std::vector<LazyArgs> la;
};

template <int CH, bool LDS_STATE>
static int launch_batch(const ChainPlan &pl, ChainLaunch &cl, const std::vector<SolveJob> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                        hipEvent_t ev_arr_done) {
    const int n = pl.n, nl = (int)jobs.size();
    DevBuf &d_c2 = pl.args[0], &d_la = pl.args[1];
    const size_t shm_aug = cl.shm_aug, shm_lazy = cl.shm_lazy;
    int rc;
    const bool cs_lds = !LDS_STATE && n <= 65535 && !cl.no_cs_lds;
    void (*kern)(const Chain2Args *) = jv_chain2<CH, LDS_STATE, false>;
    if constexpr (!LDS_STATE) { if (cs_lds) kern = jv_chain2<CH, false, true>; }
    auto build_all_caches = [&]() -> int {
        for (const SolveJob &j : jobs) {
            const int r2 = build_caches(pl.cache, n, j.ld, j.cost, j.rowmap, j.fws, j.cache_col, j.cache_val, j.same, stream);
            if (r2) return r2;
        }
        return CYTO_OK;
    };
    std::vector<Chain2Args> &h_c2 = cl.c2;
    std::vector<LazyArgs> &h_la = cl.la;
    if (!LDS_STATE) for (LazyArgs &a : h_la) a.may_bail = 0;        // only the dense jv_aug2<CH, true> can take over
    if ((rc = d_c2.alloc(sizeof(Chain2Args) * nl, stream)) || (rc = d_la.alloc(sizeof(LazyArgs) * nl, stream))) return rc;
    CYTO_HIP(hipMemcpyAsync(d_c2.p, h_c2.data(), sizeof(Chain2Args) * nl, hipMemcpyHostToDevice, stream));
    CYTO_HIP(hipMemcpyAsync(d_la.p, h_la.data(), sizeof(LazyArgs) * nl, hipMemcpyHostToDevice, stream));

    if ((rc = build_all_caches())) return rc;
    CYTO_HIP(hipEventRecord(ev_cache_done, stream));
    if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(kern)))) return rc;
    if (cl.shm_chain > (size_t)LDS_DYNAMIC_MAX || shm_aug > (size_t)LDS_DYNAMIC_MAX || shm_lazy > (size_t)LDS_DYNAMIC_MAX) return CYTO_ERR_INTERNAL;
    hipLaunchKernelGGL(kern, dim3(nl), dim3(BLOCK2), cl.shm_chain, stream, d_c2.as<Chain2Args>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipEventRecord(ev_arr_done, stream));
    auto launch_dense = [&](const Chain2Args *d_args, int count) -> int {
        if constexpr (LDS_STATE) {
            void (*ka)(const Chain2Args *) = jv_aug2<CH, true, BLOCK2>;
            int r2 = set_max_dynamic_lds(reinterpret_cast<const void *>(ka));
            if (r2) return r2;
            hipLaunchKernelGGL(ka, dim3(count), dim3(BLOCK2), shm_aug, stream, d_args);
            CYTO_HIP(hipGetLastError());
            return CYTO_OK;
        } else {
            (void)d_args; (void)count;
            return CYTO_ERR_INTERNAL;     // (beyond the LDS-resident sizes the cache-certified search is always used)
        }
    };
    if (!cl.lazy) return launch_dense(d_c2.as<Chain2Args>(), nl);

    // fresh caches (floors against the prices the augmentation starts from), then the cache-certified search
    if ((rc = build_all_caches())) return rc;
    void (*lk)(const LazyArgs *) = cl.lz_lds_state ? jv_aug_lazy<true> : (cl.lz_cs_lds ? jv_aug_lazy<false, true> : jv_aug_lazy<false>);
    if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(lk)))) return rc;
    hipLaunchKernelGGL(lk, dim3(nl), dim3(BLOCK2), shm_lazy, stream, d_la.as<LazyArgs>());
    CYTO_HIP(hipGetLastError());
    if constexpr (LDS_STATE) {
        // which searches gave up?
        constexpr size_t h0 = offsetof(LapStatus, numfree), h1 = offsetof(LapStatus, lazy_done) + sizeof(int);
        bool any_bail = false;
        for (int k = 0; k < nl; k++) any_bail |= h_la[k].may_bail != 0;
        if (any_bail) {
            std::vector<LapStatus> h_hand((size_t)nl);      // numfree .. lazy_done of every problem
            for (int k = 0; k < nl; k++)
                CYTO_HIP(hipMemcpyAsync(reinterpret_cast<char *>(&h_hand[k]) + h0, h_c2[k].misc + h0, h1 - h0, hipMemcpyDeviceToHost, stream));
            CYTO_HIP(hipStreamSynchronize(stream));
            std::vector<Chain2Args> cont;
            for (int k = 0; k < nl; k++)
                if (h_la[k].may_bail && h_hand[k].lazy_done < h_hand[k].numfree) { Chain2Args a = h_c2[k]; a.aug_start = h_hand[k].lazy_done; cont.push_back(a); }
            if (!cont.empty()) {
                // (the first nl blocks of d_c2 are no longer read: jv_chain2 has finished)
                CYTO_HIP(hipMemcpyAsync(d_c2.p, cont.data(), sizeof(Chain2Args) * cont.size(), hipMemcpyHostToDevice, stream));
                if ((rc = launch_dense(d_c2.as<Chain2Args>(), (int)cont.size()))) return rc;
                CYTO_HIP(hipStreamSynchronize(stream));     // `cont` is read by the copy until here
            }
        }
    }
    return CYTO_OK;
}

int chain_solve_batch(const ChainPlan &pl, const std::vector<SolveJob> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                      hipEvent_t ev_arr_done) {
    const int n = pl.n, nl = (int)jobs.size();
    if (!nl) return CYTO_OK;
    int rc;
    const int per2 = 4 * BLOCK2;
    const bool force_l2 = pl.variant != 0, lds_variant = chain_lds_variant(pl);
    ChainLaunch cl;
    cl.no_cs_lds = pl.variant == 3;                    // (3: as 2, with colsol in global memory too -- what n > 65 535 uses)
    cl.lazy = chain_lazy(pl);
    const int npad = (n + 3) & ~3;
    const size_t npad6 = (((size_t)npad * 6) + 15) & ~(size_t)15, npad2 = (((size_t)npad * 2) + 15) & ~(size_t)15;
    const size_t nb24 = (size_t)((((n + 63) / 64) + 511) & ~511) * 8 + (size_t)((n + 63) / 64) * 24 + 16;
    const size_t lds_budget = LDS_DYNAMIC_MAX;
    cl.lz_lds_state = n <= 65535 && !force_l2 && npad6 + nb24 <= lds_budget;
    cl.lz_cs_lds = !cl.lz_lds_state && n <= 65535 && !cl.no_cs_lds && npad2 + nb24 <= lds_budget;
    const size_t lz_base_shm = (cl.lz_lds_state ? npad6 : (cl.lz_cs_lds ? npad2 : 0)) + nb24;
    const bool cs_lds_chain = !lds_variant && n <= 65535 && !cl.no_cs_lds;
    cl.shm_chain = lds_variant ? (((size_t)npad * 6 + 15) / 16) * 16 : (cs_lds_chain ? (((size_t)npad * 2 + 15) / 16) * 16 : 16);

    // ---- per-problem argument blocks ----
    const bool want_groups = n >= 2;
    cl.c2.resize((size_t)nl); cl.la.resize((size_t)nl);
    for (int k = 0; k < nl; k++) {
        const SolveJob &j = jobs[(size_t)k];
        float *d_v = j.fws, *d_u = d_v + n;
        int32_t *d_rowsol = j.iws, *d_colsol = d_rowsol + n, *d_free = d_rowsol + 3 * (size_t)n;
        const int ng = j.ngroups;
        Chain2Args &c2 = cl.c2[(size_t)k];
        c2.n = n; c2.ld = j.ld; c2.cost = j.cost; c2.fws = d_v; c2.iws = d_rowsol;
        c2.cache_col = j.cache_col; c2.cache_val = j.cache_val; c2.misc = j.misc;
        // duplicate-row skip: per-group state in LDS when it fits beside v (4 B) and colsol (2 B) per column
        c2.rowgid = const_cast<int32_t *>(j.rowgid); c2.ngroups = ng; c2.gmode = 0; c2.g_hbest = nullptr; c2.g_hstamp = nullptr;
        c2.auxlds = 0; c2.aug_start = 0;
        c2.rowmap = j.rowmap;
        LazyArgs &la = cl.la[(size_t)k];
        memset(&la, 0, sizeof la);
        size_t shm_lazy = lz_base_shm;
        if (cl.lazy) {
            la.n = n; la.ld = j.ld; la.cost = j.cost; la.gv = d_v; la.gu = d_u; la.sumvd = d_v + 2 * (int64_t)n;
            la.cassign = d_v + 3 * (int64_t)n; la.dkey = reinterpret_cast<uint64_t *>(d_v + 4 * (int64_t)n);
            la.rowsol = d_rowsol; la.colsol = d_colsol; la.freerows = d_free;
            la.srow = d_rowsol + 6 * (int64_t)n;      // [n+1]: runs into the next slot, which the lazy path does not use
            la.slist = d_rowsol + 8 * (int64_t)n; la.slevel = d_rowsol + 9 * (int64_t)n;
            la.rowgid = j.rowgid; la.cache_col = j.cache_col; la.cache_val = j.cache_val;
            la.rowmap = j.rowmap;
            la.misc = j.misc; la.ngroups = ng; la.gmode = 0; la.g_hbest = nullptr; la.g_hstamp = nullptr;
            la.may_bail = pl.no_handover ? 0 : 1;     // (launch_batch clears it where no dense kernel can take over)
            la.debug_exc = pl.inject_exceptions;
            if (want_groups && ng < n) {
                if (!pl.group_state_global && shm_lazy + (size_t)ng * 8 <= lds_budget) { la.gmode = 1; shm_lazy += (size_t)ng * 8; }
                else {
                    la.gmode = 2;
                    if ((rc = j.state[ST_LZHB].alloc((size_t)ng * 4, stream)) || (rc = j.state[ST_LZHS].alloc((size_t)ng * 4, stream))) return rc;
                    CYTO_HIP(hipMemsetAsync(j.state[ST_LZHS].p, 0, (size_t)ng * 4, stream));
                    la.g_hbest = j.state[ST_LZHB].as<float>(); la.g_hstamp = j.state[ST_LZHS].as<int32_t>();
                }
            }
        }
        if (want_groups && ng < n) {
            // LDS beside the group state: v (4 B) + colsol (2 B) per column on the LDS-resident path
            const size_t lds_state = lds_variant ? (size_t)npad * 6 : (size_t)((n + 31) / 32) * 4;
            if (!pl.group_state_global && lds_state + (size_t)ng * 8 + 8192 <= 160 * 1024) c2.gmode = 1;
            else {
                c2.gmode = 2;
                if ((rc = j.state[ST_GHB].alloc((size_t)ng * 4, stream)) || (rc = j.state[ST_GHS].alloc((size_t)ng * 4, stream))) return rc;
                CYTO_HIP(hipMemsetAsync(j.state[ST_GHS].p, 0, (size_t)ng * 4, stream));
                c2.g_hbest = j.state[ST_GHB].as<float>(); c2.g_hstamp = j.state[ST_GHS].as<int32_t>();
            }
        }
        // dense augmentation: its LDS (prices, colsol, per-group state, and the per-column auxiliaries when they fit)
        const size_t base_aug = (((lds_variant ? (size_t)npad * 6 : 0) + (c2.gmode == 1 ? (size_t)ng * 8 : 0) + 15) / 16) * 16;
        c2.auxlds = (!pl.aux_state_global && lds_variant && ng < 65536 && base_aug + (size_t)npad * 6 + 4096 <= 160 * 1024) ? 1 : 0;
        cl.shm_aug = std::max(cl.shm_aug, base_aug + (c2.auxlds ? (size_t)npad * 6 : 0) + 32);
        cl.shm_lazy = std::max(cl.shm_lazy, shm_lazy);
    }

    // ---- the launches: jv_chain2's columns per lane by size, prices and colsol in LDS where they fit ----
    if (pl.variant >= 2) return launch_batch<0, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (force_l2 && n <= 5 * per2) return launch_batch<5, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (force_l2 && n <= 16 * per2) return launch_batch<16, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (force_l2) return launch_batch<0, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (n <= 2 * per2) return launch_batch<2, true>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (n <= 5 * per2) return launch_batch<5, true>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (n <= 10 * per2) return launch_batch<10, true>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (n <= 13 * per2) return launch_batch<13, true>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    if (n <= 16 * per2) return launch_batch<16, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);
    return launch_batch<0, false>(pl, cl, jobs, stream, ev_cache_done, ev_arr_done);   // streaming dense refresh, any n
}

void chain_info(cyto_lap_info *info, const ChainPlan &pl, const LapStatus &h) {
    info->dense_refreshes = h.counters[C2_DENSE_REFRESH];
    info->aug_scans_skipped = h.counters[C2_AUG_SKIPPED];
    info->aug_dense_scans = h.counters[C2_AUG_DENSE];
    info->aug_sparse_inits = h.counters[C2_AUG_SPARSE_INIT];
    info->aug_handover = (chain_lazy(pl) && h.lazy_done < h.numfree) ? h.lazy_done : -1;
}

}  // namespace cyto
