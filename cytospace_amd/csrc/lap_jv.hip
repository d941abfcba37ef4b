// lap_jv.hip -- Jonker-Volgenant LAP solver for gfx950 (MI355X), hand-written HIP.
//
// Replaces the reference's single third-party call
//     `_, y, _ = lapjv.lapjv(cost_scaled)`
// (/root/reference/cytospace/linear_assignment_solvers/linear_assignment_solvers.py:34-40).
// Same four phases, same operand order and the same lowest-index tie-breaking as the CPU
// oracle (oracle/jv_oracle_impl.h), so rowsol/colsol/u/v are bit-identical to it.
//
// Kernel plan (float32 path; DESIGN.md section 4.1 has the exactness arguments and the measurements)
//   colred_partial / colred_finish / colred_assign : COLUMN REDUCTION.  The only phase with N^2 independent
//       work: a full-chip streaming pass (float4 per lane, >= 2k workgroups).
//   rows_same_as_prev / rows_group_ids : runs of bitwise identical rows (CytoSPACE repeats every spot row
//       slots[s] times); used to elide provably useless scans in the augmentation.
//   build_row_caches_wave / replicate_group_caches : per row, the <= 63 columns with the smallest reduced cost
//       plus a floor that bounds every other column (a certificate while prices only decrease).
//   jv_chain2<CH, LDS_STATE> : REDUCTION TRANSFER + AUGMENTING ROW REDUCTION, a chain of dependent row scans.
//       One persistent 512-thread workgroup; a scan is served from the row's cache by wave 0 alone whenever the
//       cache certifies its top-2, otherwise the workgroup re-scans the row (refresh_row / refresh_row_stream).
//   jv_aug_lazy<LDS_STATE> (n > 5120) : AUGMENTATION with cache-certified scans and sparse search initialisation.
//   jv_aug2<CH, LDS_STATE> (n <= 5120, and taking over from jv_aug_lazy on deep searches) : dense augmentation,
//       per-column search state in registers.
// The float64 solver (jv_chain<T, CH>, jv_chain_stream) is lap_f64.hip, the float64 certificate and the exact option lap_exact.hip,
// the wide solver -- what runs by default -- lap_wide.hip; this file also holds the float32 batch driver (lap_solve_f32_batch) that
// all of them hang from, and the C entry points.
//
// Compile with -ffp-contract=off (build.py does): the arithmetic is subtract/compare only,
// but nothing may be re-associated.
#include "cyto_common.h"
#include "lap_dev.h"
#include "lap_chain.h"
#include "lap_exact.h"
#include "lap_wide.h"
#include <math.h>
#include <atomic>
#include <cmath>
#include <type_traits>
#include <vector>
#include <algorithm>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

namespace cyto {

// COLUMN REDUCTION, the last step (colred_partial / colred_finish: lap_chain.h)
__global__ void colred_assign(int n, const int32_t *__restrict__ imin, const int32_t *__restrict__ rowsol,
                              int32_t *__restrict__ colsol) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int i = imin[j];
    colsol[j] = (rowsol[i] == j) ? i : -1;
}

void launch_colred_assign(int n, const int32_t *imin, const int32_t *rowsol, int32_t *colsol, hipStream_t stream) {
    hipLaunchKernelGGL(colred_assign, dim3((n + 255) / 256), dim3(256), 0, stream, n, imin, rowsol, colsol);
}

// ------------------------------------------------------------------------------------------
// Duplicate-row groups.  CytoSPACE repeats every spot row slots[s] times
// (linear_assignment_solvers.py:63-66), so the LAP often has runs of bitwise identical rows.
// same_prev[i] = 1 iff row i equals row i-1 bit for bit (early exit on the first differing 4 KiB:
// distinct rows cost one chunk, identical rows one full read).  Used by the augmentation to skip
// scans that provably change nothing (see chain_augment).
// ------------------------------------------------------------------------------------------
// with a row map: consecutive LAP rows that read the same stored row
__global__ __launch_bounds__(256) void rows_same_from_map(int n, const int32_t *__restrict__ rowmap, int32_t *__restrict__ same_prev) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) same_prev[i] = (i > 0 && rowmap[i] == rowmap[i - 1]) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(256) void rows_same_as_prev(int n, int64_t ld, const T *__restrict__ cost, int32_t *__restrict__ same_prev) {
    using V = typename VecOf<T>::type;
    constexpr int VW = VecOf<T>::W;
    __shared__ int s_diff;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        if (i == 0) { if (threadIdx.x == 0) same_prev[0] = 0; continue; }
        const V *a = reinterpret_cast<const V *>(cost + (int64_t)i * ld);
        const V *b = reinterpret_cast<const V *>(cost + (int64_t)(i - 1) * ld);
        const int nv = (n + VW - 1) / VW;
        int diff = 0;
        for (int q0 = 0; q0 < nv; q0 += 256) {
            const int q = q0 + threadIdx.x;
            bool d = false;
            if (q < nv) {
                const V x = a[q], y = b[q];
#pragma unroll
                for (int e = 0; e < VW; e++)
                    if (q * VW + e < n) d |= memcmp_neq(vec_get<T>(x, e), vec_get<T>(y, e));
            }
            if (threadIdx.x == 0) s_diff = 0;
            __syncthreads();
            if (d) s_diff = 1;
            __syncthreads();
            diff = s_diff;
            __syncthreads();
            if (diff) break;
        }
        if (threadIdx.x == 0) same_prev[i] = diff ? 0 : 1;
    }
}

// gid[i] = number of group starts in rows 0..i, minus 1; *ngroups = number of groups (one workgroup)
__global__ __launch_bounds__(1024) void rows_group_ids(int n, const int32_t *__restrict__ same_prev, int32_t *__restrict__ gid,
                                                       int *__restrict__ ngroups) {
    __shared__ int s_part[1024];
    const int tid = threadIdx.x;
    const int R = (n + 1023) / 1024;
    const int r0 = min(n, tid * R), r1 = min(n, r0 + R);
    int c = 0;
    for (int i = r0; i < r1; i++) c += same_prev[i] ? 0 : 1;
    s_part[tid] = c;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int y = tid >= off ? s_part[tid - off] : 0;
        __syncthreads();
        s_part[tid] += y;
        __syncthreads();
    }
    int run = s_part[tid] - c;
    for (int i = r0; i < r1; i++) { run += same_prev[i] ? 0 : 1; gid[i] = run - 1; }
    if (tid == 1023) *ngroups = s_part[1023];
}

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

#define SLOT_COL(sl) ((((sl) / 4) * BLOCK2 + tid) * 4 + ((sl) % 4))

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
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
        if ((validm >> sl) & 1) k2_push(loc, mkkey(HVAL(sl), (uint32_t)SLOT_COL(sl)));
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
                    ccol[pos] = (uint32_t)SLOT_COL(sl);
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

// Runs of bitwise identical consecutive rows (same_prev[i] = row i equals row i - 1: rows_same_as_prev / rows_same_from_map --
// CytoSPACE repeats every spot row slots[s] times) have identical caches: the build kernels make the cache of the first row of
// every run, this one copies it to the others (a wave per run; c3: ten rows per spot -- a tenth of the cache-build work).
__global__ __launch_bounds__(256) void replicate_group_caches(int n, const int32_t *__restrict__ same_prev, uint32_t *__restrict__ cache_col,
                                                               float *__restrict__ cache_val) {
    // a wave per DESTINATION row (a copy of the row before it): its run's first row is found 64 rows at a time (lane l looks at row
    // i - l), so a long run -- one spot with thousands of slots, a constant matrix -- is copied by as many waves as it has rows
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    for (int i = gw; i < n; i += nw) {
        if (!same_prev[i]) continue;                                       // the first row of its run: built, not copied
        int f = -1;
        for (int base = i; f < 0; base -= 64) {
            const int r = base - lane;
            const uint64_t starts = __ballot(r >= 0 && !same_prev[r]);    // (row 0 always starts a run)
            if (starts) f = base - (__ffsll((unsigned long long)starts) - 1);
        }
        cache_col[(int64_t)i * KC + lane] = cache_col[(int64_t)f * KC + lane];
        cache_val[(int64_t)i * KC + lane] = cache_val[(int64_t)f * KC + lane];
    }
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

// ------------------------------------------------------------------------------------------------------------------------------
// The full-chip cache build as ONE WAVE PER ROW (round 4; what the build before and between the solver's phases runs).  The
// round-3 builders were a workgroup per row over refresh_row / refresh_row_stream: a row in 187 VGPRs (CH = 10: one workgroup per
// CU, its loads never overlap its threshold search -- 2.1 TB/s at n = 20 000) or swept several times between workgroup barriers
// (the streaming form: 3.0 TB/s at n = 50 000); git history has them.  Here a wave streams its row ONCE with U quads per lane in flight and no barrier anywhere.  Rows of >= 256 U columns: a streaming
// selection without a guess (cb_stream below: the columns under a falling threshold are compacted into a 768-byte staging line of the
// wave by ballot as they pass).  Shorter rows, and rows the selection gives up on (ties, an adversarial column order): the floor is
// guessed (the floor of the wave's previous row; ANY floor that admits <= 63 columns makes a valid cache) and the columns under it are
// staged during the sweep; a guess that does not fit is replaced by the 35th smallest of the row's 64 lane minima (49 +- 5 columns lie
// below it whatever the distribution) and the (L2 / MALL resident) row is swept again; a bisection as before when that fails too.
// Same cache contract as refresh_row.
constexpr int CBW = 4;             // waves per workgroup (they share nothing but the launch)
struct CbStage { uint32_t col[KC]; float val[KC]; float h[KC]; };

// one sweep of the row: counts the columns with h < tau and stages the first 64 of them; TRACK: also the lane minima
template <int U, bool TRACK>
__device__ __forceinline__ int cb_sweep(const __amdgpu_buffer_rsrc_t rrow, const __amdgpu_buffer_rsrc_t rv, const float *__restrict__ row,
                                        const float *__restrict__ v, int n, int lane, float tau, float &lmin, CbStage &st) {
    const int nfull = n >> 2, ntail = n & 3;
    const uint64_t lt = (1ull << lane) - 1ull;
    int cnt = 0;
    auto one = [&](uint32_t c, float raw, bool p) {                // (convergent: every lane of the wave calls it)
        const uint64_t m = __ballot(p);
        if (m) {
            const int pos = cnt + __popcll(m & lt);
            if (p && pos < KC) { st.col[pos] = c; st.val[pos] = raw; }
            cnt += __popcll(m);
        }
    };
    auto quad = [&](int q, const u32x4_t &xr, const u32x4_t &vr, bool inrange) {
        const float r0 = __uint_as_float(xr.x), r1 = __uint_as_float(xr.y), r2 = __uint_as_float(xr.z), r3 = __uint_as_float(xr.w);
        const float h0 = r0 - __uint_as_float(vr.x), h1 = r1 - __uint_as_float(vr.y), h2 = r2 - __uint_as_float(vr.z),
                    h3 = r3 - __uint_as_float(vr.w);
        float m4 = fminf(fminf(h0, h1), fminf(h2, h3));
        if (!inrange) m4 = INFINITY;
        if (TRACK) lmin = fminf(lmin, m4);
        if (__ballot(m4 < tau)) {
            const uint32_t c0 = (uint32_t)q * 4u;
            one(c0, r0, inrange && h0 < tau); one(c0 + 1, r1, inrange && h1 < tau);
            one(c0 + 2, r2, inrange && h2 < tau); one(c0 + 3, r3, inrange && h3 < tau);
        }
    };
    int base = 0;
    for (; base + 64 * U <= nfull; base += 64 * U) {                // (wave-uniform trips; all U quads of every lane in range)
        u32x4_t xr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xr[u] = __builtin_amdgcn_raw_buffer_load_b128(rrow, (base + 64 * u + lane) * 16, 0, 0);
            vr[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, (base + 64 * u + lane) * 16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; u++) quad(base + 64 * u + lane, xr[u], vr[u], true);
    }
    for (; base < nfull; base += 64) {                               // (reads past the descriptors' extents give zeros)
        const int q = base + lane;
        const u32x4_t xr = __builtin_amdgcn_raw_buffer_load_b128(rrow, q * 16, 0, 0);
        const u32x4_t vr = __builtin_amdgcn_raw_buffer_load_b128(rv, q * 16, 0, 0);
        quad(q, xr, vr, q < nfull);
    }
    if (ntail) {                                                     // the ragged last quad: a column per lane
        const int c = nfull * 4 + lane;
        const bool valid = lane < ntail;
        const float raw = valid ? row[c] : 0.0f;
        const float h = valid ? raw - v[c] : INFINITY;
        if (TRACK) lmin = fminf(lmin, h);
        one((uint32_t)c, raw, valid && h < tau);
    }
    return cnt;
}

// ascending bitonic sort of one float per lane
__device__ __forceinline__ float cb_sort64(float x, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const float o = __shfl_xor(x, j);
            const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
            x = take_min ? fminf(x, o) : fmaxf(x, o);
        }
    }
    return x;
}
// the staged set (cnt <= 64 entries) cut down to the columns below its (K + 1)-th smallest reduced cost, which becomes the threshold
__device__ __forceinline__ void cb_compress(CbStage &st, int lane, int K, int &cnt, float &T) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t c = lane < cnt ? st.col[lane] : COLSENT;
    const float r = lane < cnt ? st.val[lane] : 0.0f;
    const float h = lane < cnt ? st.h[lane] : INFINITY;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float srt = cb_sort64(h, lane);
    const float Tn = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(srt), K));
    if (!(Tn < INFINITY)) return;                                  // no more than K entries: nothing to drop
    T = Tn;
    const bool keep = h < Tn;
    const uint64_t m = __ballot(keep);
    if (keep) { const int p = __popcll(m & ((1ull << lane) - 1ull)); st.col[p] = c; st.val[p] = r; st.h[p] = h; }
    cnt = __popcll(m);
}

// The row in ONE sweep without a guess (rows of >= 256 U columns): the first U quads of every lane (read twice) give 64 lane minima, the 17th
// smallest of them (in a long row; up to the 35th in a row of little more than 256 U columns) is the first threshold T (~19 of those
// 256 U columns lie below it, whatever the distribution); from then on every
// column below T is staged as it passes, and when the 64 staging slots run over the staged set is cut down to the columns below its
// 25th smallest reduced cost, which becomes T (a streaming selection: T only falls, so nothing that was passed over could qualify
// later; two or three cuts per row, each keeping what leaves ~54 columns at the row's end).  At the end the stage holds EVERY column
// below T, 16 ... 63 of them (~52 on average).  false: the slots
// ran over twice in one step (an adversarial order of the columns) or fewer than 16 columns are left (ties) -- the caller falls
// back on the sweeps of the search above, for which the lane minima of the whole row are returned in any case.
template <int U>
__device__ __forceinline__ bool cb_stream(const __amdgpu_buffer_rsrc_t rrow, const __amdgpu_buffer_rsrc_t rv, const float *__restrict__ row,
                                          const float *__restrict__ v, int n, int lane, float &T_out, int &cnt_out, float &lmin, CbStage &st) {
    const int nfull = n >> 2, ntail = n & 3;
    const uint64_t lt = (1ull << lane) - 1ull;
    int cnt = 0, base = 0;                                           // base: the quad the sweep has reached (wave-uniform)
    float T = INFINITY;
    bool fail = false;
    auto one = [&](uint32_t c, float raw, float h, bool valid) {     // (convergent: every lane of the wave calls it)
        bool p = valid && h < T;
        uint64_t m = __ballot(p);
        if (!m) return;
        if (cnt + __popcll(m) > KC) {
            // how many to keep: the columns still to come bring K (n - m) / m more below the new threshold when m columns have passed
            // (any order of the columns but an adversarial one), so K = 54 m / n leaves ~54 at the end of the row -- a cut early in
            // the row is a deep one, but never below 24: the threshold that leaves 8 of 7 000 columns is known to +-35 %, and rows ended
            // with anything from 25 to 63 columns (50 000^2: 356 full-row bids instead of 146).  (Cutting to 24 wherever the slots ran over left 16 ... 63, 40 on average: the build was faster
            // and the solve slower -- 50 000^2: 1 585 instead of 146 full-row bids, row reduction 20.5 -> 25 ms.)
            const int K = (int)min(48ll, max(24ll, 54ll * (4ll * base) / (long long)n));
            cb_compress(st, lane, K, cnt, T);
            p = p && h < T;
            m = __ballot(p);
            if (!m) return;
            if (cnt + __popcll(m) > KC) { fail = true; return; }
        }
        if (p) { const int pos = cnt + __popcll(m & lt); st.col[pos] = c; st.val[pos] = raw; st.h[pos] = h; }
        cnt += __popcll(m);
    };
    auto quad = [&](int q, const u32x4_t &xr, const u32x4_t &vr, bool inrange) {
        const float r0 = __uint_as_float(xr.x), r1 = __uint_as_float(xr.y), r2 = __uint_as_float(xr.z), r3 = __uint_as_float(xr.w);
        const float h0 = r0 - __uint_as_float(vr.x), h1 = r1 - __uint_as_float(vr.y), h2 = r2 - __uint_as_float(vr.z),
                    h3 = r3 - __uint_as_float(vr.w);
        float m4 = fminf(fminf(h0, h1), fminf(h2, h3));
        if (!inrange) m4 = INFINITY;
        lmin = fminf(lmin, m4);
        if (__ballot(m4 < T)) {
            const uint32_t c0 = (uint32_t)q * 4u;
            one(c0, r0, h0, inrange); one(c0 + 1, r1, h1, inrange); one(c0 + 2, r2, h2, inrange); one(c0 + 3, r3, h3, inrange);
        }
    };
    {   // the first U quads of every lane: lane minima and the first threshold; the sweep below starts over with them (8 KB that the
        // wave has just read: keeping them in registers across the sort cost a third of the occupancy)
        float m0 = INFINITY;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const u32x4_t xr = __builtin_amdgcn_raw_buffer_load_b128(rrow, (64 * u + lane) * 16, 0, 0);
            const u32x4_t vr = __builtin_amdgcn_raw_buffer_load_b128(rv, (64 * u + lane) * 16, 0, 0);
            m0 = fminf(m0, fminf(fminf(__uint_as_float(xr.x) - __uint_as_float(vr.x), __uint_as_float(xr.y) - __uint_as_float(vr.y)),
                                 fminf(__uint_as_float(xr.z) - __uint_as_float(vr.z), __uint_as_float(xr.w) - __uint_as_float(vr.w))));
        }
        const float srt = cb_sort64(m0, lane);
        // which lane minimum: ~c0 of the first 256 U columns are wanted below it, c0 = 54 * 256 U / n (the rest of the row brings its
        // share), 18 at least and 49 at most (a row of just 256 U columns: the 35th smallest, the two-sweep form's choice); c columns lie
        // below the (i + 1)-th smallest of 64 lane minima for i = 64 (1 - exp(-(c + 1) / 64)) (the draws it takes to hit i + 1 lanes)
        const float c0 = fminf(49.0f, fmaxf(18.0f, 54.0f * (float)(256 * U) / (float)n));
        const int i0 = __builtin_amdgcn_readfirstlane((int)(64.0f * (1.0f - __expf(-(c0 + 1.0f) * 0.015625f))));
        T = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(srt), i0));
    }
    for (; base + 64 * U <= nfull; base += 64 * U) {
        u32x4_t xr[U], vr[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            xr[u] = __builtin_amdgcn_raw_buffer_load_b128(rrow, (base + 64 * u + lane) * 16, 0, 0);
            vr[u] = __builtin_amdgcn_raw_buffer_load_b128(rv, (base + 64 * u + lane) * 16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < U; u++) quad(base + 64 * u + lane, xr[u], vr[u], true);
    }
    for (; base < nfull; base += 64) {
        const int q = base + lane;
        const u32x4_t xr = __builtin_amdgcn_raw_buffer_load_b128(rrow, q * 16, 0, 0);
        const u32x4_t vr = __builtin_amdgcn_raw_buffer_load_b128(rv, q * 16, 0, 0);
        quad(q, xr, vr, q < nfull);
    }
    if (ntail) {
        const int c = nfull * 4 + lane;
        const bool valid = lane < ntail;
        const float raw = valid ? row[c] : 0.0f;
        const float h = valid ? raw - v[c] : INFINITY;
        lmin = fminf(lmin, h);
        one((uint32_t)c, raw, h, valid);
    }
    if (!fail && cnt > KCU) cb_compress(st, lane, 48, cnt, T);     // (64 staged: the cache has 63 slots)
    T_out = T; cnt_out = cnt;
    return !fail && cnt <= KCU && cnt >= 16 && T < INFINITY;
}

template <int U>
__global__ __launch_bounds__(64 * CBW) void build_row_caches_wave(int n, int64_t ld, const float *__restrict__ cost,
                                                                 const float *__restrict__ v, uint32_t *__restrict__ cache_col,
                                                                 float *__restrict__ cache_val, const int32_t *__restrict__ rowmap,
                                                                 const int32_t *__restrict__ same_prev, int stream,
                                                                 const int32_t *__restrict__ rowlist, int count) {
    // rowlist (or null: all n rows): the `count` rows to build, in any order -- a wave takes list positions where it takes row indices
    __shared__ CbStage stage[CBW];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (scalar: row bases and descriptors stay in SGPRs)
    CbStage &st = stage[w];
    const int gw = (int)blockIdx.x * CBW + w, nw = (int)gridDim.x * CBW;
    const int nrows = rowlist ? count : n;
    const int per = (nrows + nw - 1) / nw, i_end = min(nrows, (gw + 1) * per);      // (a contiguous range of rows per wave)
    const int nquad = (n + 3) >> 2;
    const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(v), 0, nquad * 16, 0x00020000);
    float tau_guess = INFINITY, delta = 0.0f;
    for (int ii = gw * per; ii < i_end; ii++) {
        const int i = rowlist ? __builtin_amdgcn_readfirstlane(rowlist[ii]) : ii;
        if (same_prev && same_prev[i]) continue;                          // a copy of the previous row: replicate_group_caches
        const float *__restrict__ row = cost + row_off(rowmap, i, ld);
        const __amdgpu_buffer_rsrc_t rrow = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(row), 0, (int)(ld * 4), 0x00020000);
        float tau0 = tau_guess;
        float lmin = INFINITY, dummy = 0.0f, tau = tau0;
        int cnt = 0;
        bool have = false;
        if (stream && (n >> 2) >= 64 * U) {                                // one sweep, no guess (cb_stream); else the lane minima are complete
            have = cb_stream<U>(rrow, rv, row, v, n, lane, tau, cnt, lmin, st);
            if (!have) { tau0 = INFINITY; tau = INFINITY; cnt = 0; }
        } else {
            cnt = cb_sweep<U, true>(rrow, rv, row, v, n, lane, tau0 < INFINITY ? tau0 : -INFINITY, lmin, st);
            have = tau0 < INFINITY && cnt <= KCU && (cnt >= KCU / 2 || cnt >= n);      // the guess fits: one sweep
        }
        if (!have) {
            const float umin = ord2f(wave_min_u32(f2ord(lmin)));
            float lo = 0.0f, hi = INFINITY;
            bool okc = false;
            {   // the 35th smallest of the 64 lane minima: 49 +- 5 columns lie below it whatever the distribution (distinct values;
                //  lap_wide.hip, SC_FLOOR_POS) -- the bisection that follows is for rows with ties
                float lm = lmin;
#pragma unroll
                for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
                    for (int j = k >> 1; j > 0; j >>= 1) {
                        const float o = __shfl_xor(lm, j);
                        const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                        lm = take_min ? fminf(lm, o) : fmaxf(lm, o);
                    }
                }
                const float m34 = __shfl(lm, 34);
                if (m34 < INFINITY && m34 > umin) delta = m34 - umin;
                else if (tau0 < INFINITY && tau0 > umin && cnt > 0) {     // (fewer than 35 lanes have columns) scale the guess by its count
                    const float d0 = tau0 - umin;
                    if (cnt > KCU) { hi = d0; delta = d0 * fmaxf(0.0625f, 0.75f * (float)KCU / (float)cnt); }
                    else { lo = d0; delta = d0 * fminf(16.0f, 0.75f * (float)KCU / (float)cnt); }
                }
            }
            if (!(delta > 0.0f) || !(delta < 1e30f)) delta = 1e-3f;
            for (int it = 0; it < 24 && !okc; it++) {
                tau = umin + delta;
                cnt = cb_sweep<U, false>(rrow, rv, row, v, n, lane, tau, dummy, st);
                if (cnt > KCU) {
                    hi = delta;
                    const float mid = (lo > 0.0f) ? 0.5f * (lo + hi) : 0.5f * delta;
                    if (!(mid < hi) || !(mid > lo)) break;               // cannot separate: too many ties just above umin
                    delta = mid;
                } else if (cnt < KCU / 2 && cnt < n && delta < 1e30f) {
                    lo = delta;
                    const float mid = (hi < INFINITY) ? 0.5f * (lo + hi) : 2.0f * delta;
                    if (hi < INFINITY && (!(mid < hi) || !(mid > lo))) { okc = true; break; }      // best separable threshold
                    delta = mid;
                } else {
                    okc = true;
                }
            }
            if (!okc || cnt > KCU) {
                // the largest threshold known to admit <= KCU columns (possibly none), staged once more
                if (lo > 0.0f) { delta = lo; tau = umin + lo; } else { tau = -INFINITY; }
                cnt = cb_sweep<U, false>(rrow, rv, row, v, n, lane, tau, dummy, st);
                if (cnt > KCU) { tau = -INFINITY; cnt = 0; }
            }
        }
        tau_guess = tau > -INFINITY ? tau : INFINITY;
        // the staged columns, sorted by column (unused slots last), the floor in slot 63
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t kc = lane < cnt ? st.col[lane] : COLSENT;
        float kv = lane < cnt ? st.val[lane] : 0.0f;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
            for (int j = k >> 1; j > 0; j >>= 1) {
                const uint32_t pk = (uint32_t)__shfl_xor((int)kc, j);
                const float pv = __shfl_xor(kv, j);
                const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
                const bool sw = take_min ? (pk < kc) : (pk > kc);
                kc = sw ? pk : kc; kv = sw ? pv : kv;
            }
        }
        if (lane == KCU) { kc = COLSENT; kv = tau; }               // (at most 63 entries: lane 63 held a sentinel)
        cache_col[(int64_t)i * KC + lane] = kc;
        cache_val[(int64_t)i * KC + lane] = kv;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// FIRST caches from the column reduction's own pass (float32, the wide solver, no row map).  The column reduction
// and the first cache build each stream the whole matrix, for a result that needs every entry once.  Here the column pass lists,
// per row, the few hundred columns that can be in the row's cache (colred_partial_append), against an UPPER bound w of
// the prices (fused_w: the column minima over the first rows) and a per-row threshold theta (fused_theta); when the prices v exist,
// fused_fixup turns each list into an ordinary cache.  Exact: w >= v and rounding is monotone, so fl(c - v[j]) >= fl(c - w[j]);
// the list { j : fl(c - w[j]) < theta } therefore holds EVERY column with fl(c - v[j]) < theta, and any floor tau <= theta with at
// most 63 listed columns below it gives the cache { j : fl(c - v[j]) < tau }, floor tau.  Rows the lists cannot certify (list over
// its cap, fewer than min_kept columns below tau) go on a row list for build_row_caches_wave.  min_kept (fused_min_kept) is 48 from
// 4 096 columns on, not the contract's 16: the row reduction pays for every thin cache with full-row bids (50 000^2: rows accepted
// from 16 columns on -- 3 % of them end below 63 -- 240 full-row bids and 41.7 ms a solve; from 48 on 3 bids and 38.3 ms; the row
// builder's own caches 79 bids and 39.8 ms).
constexpr int FUSED_S = 2048;       // columns of a row that fused_theta reads (64 lanes x 8 quads)
constexpr int FUSED_TARGET = 190;   // listed columns per row aimed at
constexpr int COLRED_CAP = 512;     // entries of a row's candidate list
struct ColredAppend {
    const float *w; const float *theta;
    int32_t *cnt; uint2 *list;      // [n], [n][COLRED_CAP]
};
// colred_partial (lap_chain.h) for float32 without a row map, which also LISTS the candidates: every column with
// fl(c - w[j]) < theta[r] is appended to list[r] as (column, raw cost bits).  A wave whose ballot shows a hit takes ONE returning
// atomicAdd on cnt[r] for that row; its lanes take positions by ballot prefix and store while the position is below COLRED_CAP (cnt
// keeps counting: a row over the cap is built by the row builder instead).  Column minima, the lowest row on ties, the non-finite
// flag and pmin / parg are colred_partial's.  Every lane stays for the ballots: past the last quad it re-reads that quad and owns no
// column.
__global__ __launch_bounds__(256) void colred_partial_append(int n, int64_t ld, const float *__restrict__ cost, int rows_per_block,
                                                             float *__restrict__ pmin, int32_t *__restrict__ parg,
                                                             int *__restrict__ nonfinite, int nrows, ColredAppend ap) {
    constexpr int VW = 4, RU = 4;                                      // RU: rows of a group (two groups in flight per wave)
    const int q = blockIdx.x * 256 + threadIdx.x;                      // vector-column index
    const int col0 = q * VW, ql = min(q, (n - 1) >> 2);
    const int r0 = blockIdx.y * rows_per_block;
    const int r1 = min(nrows, r0 + rows_per_block);
    const int lane = threadIdx.x & 63;
    const uint64_t lt = (1ull << lane) - 1ull;
    float mn[VW], we[VW];
    int32_t arg[VW];
    bool bad = false;
#pragma unroll
    for (int e = 0; e < VW; e++) { mn[e] = INFINITY; arg[e] = r0; we[e] = col0 + e < n ? ap.w[col0 + e] : 0.0f; }
    // RU rows at a time, one group ahead: the NEXT group's loads are issued first, then this group's hits are found and lanes
    // 0 .. RU - 1 take the atomics of its RU rows in ONE instruction, so that the wait for their positions is also the wait for
    // the next group's loads (the latencies overlap); then the stores go out.  With stores outstanding beside loads a wave can
    // only wait for everything, so the group's registers are touched (the empty asm) BEFORE the next loads are issued: that wait
    // finds nothing but the last stores.  Past the block's last row the last row is read again, with a threshold nothing lies
    // below (a row seen twice changes no minimum).
    auto row_of = [&](int k) { return min(r0 + k, r1 - 1); };
    auto load_row = [&](int r) { return *(reinterpret_cast<const float4 *>(cost + (int64_t)r * ld) + ql); };
    float4 xn[RU]; float thn[RU];                                      // (the thresholds come with the rows: they are vector loads too)
#pragma unroll
    for (int u = 0; u < RU; u++) { xn[u] = load_row(row_of(u)); thn[u] = ap.theta[row_of(u)]; }
    for (int k = 0; r0 + k < r1; k += RU) {
        float4 x[RU]; float thr[RU]; int rr[RU];
#pragma unroll
        for (int u = 0; u < RU; u++) {
            x[u] = xn[u]; thr[u] = thn[u]; rr[u] = row_of(k + u);
            asm volatile("" : "+v"(x[u].x), "+v"(x[u].y), "+v"(x[u].z), "+v"(x[u].w), "+v"(thr[u]) :: "memory");
        }
#pragma unroll
        for (int u = 0; u < RU; u++) { xn[u] = load_row(row_of(k + RU + u)); thn[u] = ap.theta[row_of(k + RU + u)]; }
        uint64_t b[RU][VW]; int tot[RU];
        int my_tot = 0, my_row = 0;
#pragma unroll
        for (int u = 0; u < RU; u++) {
            tot[u] = 0;
            const float th = r0 + k + u < r1 ? thr[u] : -INFINITY;
#pragma unroll
            for (int e = 0; e < VW; e++) {
                const float xe = vec_get<float>(x[u], e);
                if (col0 + e < n) bad |= !__builtin_isfinite(xe);
                if (xe < mn[e]) { mn[e] = xe; arg[e] = rr[u]; }
                b[u][e] = __ballot(col0 + e < n && xe - we[e] < th);
                tot[u] += __popcll(b[u][e]);
            }
            if (lane == u) { my_tot = tot[u]; my_row = rr[u]; }
        }
        uint32_t old = 0;
        if (my_tot) old = (uint32_t)atomicAdd(ap.cnt + my_row, my_tot);
        asm volatile("" : "+v"(old) :: "memory");                      // (the one wait: the positions and the next group's loads)
#pragma unroll
        for (int u = 0; u < RU; u++) {
            if (!tot[u]) continue;                                     // (wave-uniform)
            int pos = __builtin_amdgcn_readlane((int)old, u);
            uint2 *lst = ap.list + (int64_t)rr[u] * COLRED_CAP;
#pragma unroll
            for (int e = 0; e < VW; e++) {
                const int p = pos + __popcll(b[u][e] & lt);
                if (((b[u][e] >> lane) & 1ull) && (unsigned)p < (unsigned)COLRED_CAP)
                    lst[p] = make_uint2((uint32_t)(col0 + e), __float_as_uint(vec_get<float>(x[u], e)));
                pos += __popcll(b[u][e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < VW; e++) {
        if (col0 + e < n) {
            pmin[(int64_t)blockIdx.y * n + col0 + e] = mn[e];
            parg[(int64_t)blockIdx.y * n + col0 + e] = arg[e];
        }
    }
    if (bad) atomicOr(nonfinite, 1);
}


// columns a row must keep: half of what theta aims at below it (c0 of the first FUSED_S columns: c0 n / FUSED_S of the row), 16 ... 48
static int fused_min_kept(int n) {
    const double c0 = std::min(49.0, std::max(6.0, (double)FUSED_TARGET * FUSED_S / n));
    return (int)std::min(48.0, std::max(16.0, 0.5 * c0 * n / FUSED_S));
}

__global__ void fused_w(int n, int nblocks, const float *__restrict__ pmin, float *__restrict__ w) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    float mn = pmin[j];
    for (int b = 1; b < nblocks; b++) mn = fminf(mn, pmin[(int64_t)b * n + j]);
    w[j] = mn;
}

// theta[i]: the (i0 + 1)-th smallest of the 64 lane minima of fl(c - w) over the row's first FUSED_S columns, i0 as in cb_stream for
// c0 = FUSED_TARGET * FUSED_S / n columns wanted below it among those (6 at least, 49 at most).  n >= FUSED_S.
__global__ __launch_bounds__(256) void fused_theta(int n, int64_t ld, const float *__restrict__ cost, const float *__restrict__ w,
                                                   float *__restrict__ theta) {
    const int lane = threadIdx.x & 63, i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (i >= n) return;
    const float4 *row = reinterpret_cast<const float4 *>(cost + (int64_t)i * ld), *w4 = reinterpret_cast<const float4 *>(w);
    float m = INFINITY;
#pragma unroll
    for (int u = 0; u < FUSED_S / 256; u++) {
        const float4 x = row[64 * u + lane], y = w4[64 * u + lane];
        m = fminf(m, fminf(fminf(x.x - y.x, x.y - y.y), fminf(x.z - y.z, x.w - y.w)));
    }
    const float srt = cb_sort64(m, lane);
    const float c0 = fminf(49.0f, fmaxf(6.0f, (float)FUSED_TARGET * (float)FUSED_S / (float)n));
    const int i0 = (int)(64.0f * (1.0f - __expf(-(c0 + 1.0f) * 0.015625f)));
    const float th = __shfl(srt, i0);
    if (lane == 0) theta[i] = th;
}

// One wave per row: the row's list against the final prices.  The cache does not depend on the order of the list.
__global__ __launch_bounds__(256) void fused_fixup(int n, const float *__restrict__ v, const float *__restrict__ theta,
                                                   const int32_t *__restrict__ cnt, const uint2 *__restrict__ list,
                                                   const int32_t *__restrict__ same_prev, uint32_t *__restrict__ cache_col,
                                                   float *__restrict__ cache_val, int32_t *__restrict__ rowlist, int32_t *__restrict__ nfail,
                                                   int min_kept) {
    constexpr int NT = COLRED_CAP / 64;
    __shared__ uint32_t s_col[4][KC];
    __shared__ float s_val[4][KC];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = (int)blockIdx.x * 4 + w;
    if (i >= n) return;
    if (same_prev && same_prev[i]) return;                                // a copy of the previous row: replicate_group_caches
    const int c = __builtin_amdgcn_readfirstlane(cnt[i]);
    const uint64_t lt = (1ull << lane) - 1ull;
    float tau = theta[i];
    bool fail = c > COLRED_CAP;
    int kept = 0;
    if (!fail) {
        const int nt = (c + 63) >> 6;
        uint32_t col[NT]; float raw[NT], h[NT];
        int below = 0;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            col[t] = 0; raw[t] = 0.0f; h[t] = INFINITY;
            if (t < nt) {
                const int k = 64 * t + lane;
                if (k < c) {
                    const uint2 e = list[(int64_t)i * COLRED_CAP + k];
                    col[t] = e.x; raw[t] = __uint_as_float(e.y);
                    const float hh = raw[t] - v[e.x];
                    if (hh < tau) h[t] = hh;
                }
                below += __popcll(__ballot(h[t] < INFINITY));
            }
        }
        if (below > KCU) {
            // the 64th smallest reduced cost, as an ordered key: the largest P with at most 63 keys below it
            uint32_t key[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) key[t] = f2ord(h[t]);
            uint32_t P = 0;
            for (int bit = 31; bit >= 0; bit--) {
                const uint32_t cand = P | (1u << bit);
                int lower = 0;
#pragma unroll
                for (int t = 0; t < NT; t++) if (t < nt) lower += __popcll(__ballot(key[t] < cand));
                if (lower <= KCU) P = cand;
            }
            tau = ord2f(P);
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t < nt) {
                const bool keep = h[t] < tau;                               // (strict: ties at tau leave fewer than 63)
                const uint64_t m = __ballot(keep);
                if (keep) { const int p = kept + __popcll(m & lt); s_col[w][p] = col[t]; s_val[w][p] = raw[t]; }
                kept += __popcll(m);
            }
        }
        fail = kept < min_kept && n > 16;
    }
    if (fail) {
        if (lane == 0) rowlist[atomicAdd(nfail, 1)] = i;
        return;
    }
    // the kept columns, sorted by column (unused slots last), the floor in slot 63: the layout build_row_caches_wave leaves
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint32_t kc = lane < kept ? s_col[w][lane] : COLSENT;
    float kv = lane < kept ? s_val[w][lane] : 0.0f;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t pk = (uint32_t)__shfl_xor((int)kc, j);
            const float pv = __shfl_xor(kv, j);
            const bool take_min = ((lane & j) == 0) == ((lane & k) == 0);
            const bool sw = take_min ? (pk < kc) : (pk > kc);
            kc = sw ? pk : kc; kv = sw ? pv : kv;
        }
    }
    if (lane == KCU) { kc = COLSENT; kv = tau; }
    cache_col[(int64_t)i * KC + lane] = kc;
    cache_val[(int64_t)i * KC + lane] = kv;
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
#undef SLOT_COL
#define SLOT_COL(sl) ((((sl) / 4) * BS + tid) * 4 + ((sl) % 4))
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
        if (((validm >> sl) & 1) && st_csget<LDS_STATE>(s_cs, gcolsol, SLOT_COL(sl)) >= 0) assignedm |= (1ull << sl);
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
                            lk = umin32(lk, (uint32_t)SLOT_COL(sl) | (((assignedm >> sl) & 1) ? 0x80000000u : 0u));
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
        if ((readym >> sl) & 1) st_vset<LDS_STATE>(s_v, gv, SLOT_COL(sl), ld_f32(&sd[SLOT_COL(sl)].x) - curmin);
    __syncthreads();
#undef VM
#undef DR
#undef SLOT_COL
#define SLOT_COL(sl) ((((sl) / 4) * BLOCK2 + tid) * 4 + ((sl) % 4))
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
    for (int sl = 0; sl < NC; sl++) if (SLOT_COL(sl) < n) validm |= (1ull << sl);

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
#undef SLOT_COL
#define SLOT_COL(sl) ((((sl) / 4) * BS + tid) * 4 + ((sl) % 4))
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
    for (int sl = 0; sl < NC; sl++) if (SLOT_COL(sl) < n) validm |= (1ull << sl);
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
#undef SLOT_COL
#define SLOT_COL(sl) ((((sl) / 4) * BLOCK2 + tid) * 4 + ((sl) % 4))
#undef SLOT_COL

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

int check_opts(const cyto_lap_opts &o) {
    if (o.chain_variant < 0 || o.chain_variant > 3 || o.augmentation < 0 || o.augmentation > 2 || o.inject_exceptions < 0 ||
        o.no_handover < 0 || o.no_handover > 1)
        return CYTO_ERR_BAD_ARG;
    if (o.group_state_global < 0 || o.group_state_global > 1 || o.aux_state_global < 0 || o.aux_state_global > 1) return CYTO_ERR_BAD_ARG;
    if (o.mode < 0 || o.mode > 2 || o.wide_rounds < -1 || o.wide_groups < -1 || o.wide_groups > 32 || o.wide_rebuild < -1 ||
        o.wide_wipe < 0 || o.wide_wipe > 2048 || o.wide_par < -1 || o.wide_par > WIDE_PAR_GMAX) return CYTO_ERR_BAD_ARG;    // (wide_groups: ignored)
    if (o.cache_waves < -1 || o.cache_waves > 32 || (o.cache_unroll != 0 && o.cache_unroll != 4 && o.cache_unroll != 8) || o.cache_stream < -1 ||
        o.cache_stream > 1)
        return CYTO_ERR_BAD_ARG;
    if (o.certify < 0 || o.certify > 1 || o.polish < 0 || o.polish > 1) return CYTO_ERR_BAD_ARG;
    if (o.exact < 0 || o.exact > EXACT_SLOTS_MAX || (o.exact && o.polish)) return CYTO_ERR_BAD_ARG;
    for (int r : o.reserved) if (r != 0) return CYTO_ERR_BAD_ARG;            // (must be zero: room for later knobs without another ABI break)
    return CYTO_OK;
}

// process-wide: solves whose first caches came from the column reduction's pass, and the rows of those solves that the row builder
// swept all the same (every row of a solve that gave the lists up)
static std::atomic<long long> g_fused_solves{0}, g_fused_fallback_rows{0};

// ---- float32: one problem of a batch (all problems of a batch have the same n) ----
struct F32Job {
    // in
    const float *cost = nullptr; int64_t ld = 0; int cost_on_device = 0;
    const int32_t *rowmap_host = nullptr; int nu = 0;   // optional row map: LAP row i reads stored row rowmap[i] (nu stored rows)
    // out (host pointers, may be null)
    int32_t *rowsol = nullptr, *colsol = nullptr; float *u = nullptr, *v = nullptr; double *total = nullptr; cyto_lap_info *info = nullptr;
    int status = CYTO_OK;
    // device state
    DevBuf slab;                // ONE block per problem for the ten work buffers every solve needs (views below): a batch of 256 problems made
                                // 3 300 hipMallocs on a process's first call -- 160 ms of a 0.67-s call (round 6, bench c4_chunks.first_call_wall_s)
    DevBuf staged, b_fws, b_iws, b_imin, b_pmin, b_parg, b_misc, b_same, b_gid, b_ccol, b_cval, b_ghb, b_ghs, b_lzhb, b_lzhs;
    DevBuf b_rowmap, b_ulist, b_ufirst, b_wide;
    int nused = 0;
    const float *dcost = nullptr; int64_t dld = 0;
    int h_nonfinite = 0, h_ngroups = 0;
    // first caches from the column reduction's pass (fused_*): w | theta | cnt | rowlist | nfail views into the slab, the lists behind them
    bool fused = false; int h_fused_failed = 0;
    float *f_w = nullptr, *f_theta = nullptr; int32_t *f_cnt = nullptr, *f_rows = nullptr, *f_nfail = nullptr; uint2 *f_list = nullptr;
    LapStatus h_hand = {};      // numfree .. lazy_done, when jv_aug_lazy may have given up
    Chain2Args c2; LazyArgs la;
    size_t shm_lazy = 0, shm_aug = 0;
    bool alive() const { return status == CYTO_OK; }
    LapStatus *st() const { return b_misc.as<LapStatus>(); }
    const int32_t *rowmap() const { return rowmap_host ? b_rowmap.as<int32_t>() : nullptr; }
    const int32_t *same(int n) const { return (h_ngroups < n && n >= 2) ? b_same.as<int32_t>() : nullptr; }    // (runs of identical rows)
};

struct F32Plan {            // what depends on n (and the options) only: identical for every problem of the batch
    int n, colblocks, rowblocks, rows_per_block;
    CachePlan cache;
    bool force_l2, lds_variant, lazy, lz_lds_state, lz_cs_lds, no_cs_lds, wide;
    size_t shm_chain, lz_base_shm;
};

int build_caches(const CachePlan &cp, int n, int64_t ld, const float *cost, const int32_t *rowmap, const float *v, uint32_t *cache_col,
                 float *cache_val, const int32_t *same, hipStream_t stream, const int32_t *rowlist, int count) {
    // (a wave per row; the grid: cp.waves waves on every CU, four to a workgroup; rowlist: only those `count` rows, or null: all)
    const int nrows = rowlist ? count : n;
    const int g = std::max(1, std::min((nrows + CBW - 1) / CBW, cp.waves * cp.cus / CBW));
    if (nrows > 0 && cp.unroll == 8)                                   // (an empty list: only the runs of identical rows are copied)
        hipLaunchKernelGGL(build_row_caches_wave<8>, dim3(g), dim3(64 * CBW), 0, stream, n, ld, cost, v, cache_col, cache_val, rowmap, same,
                           cp.stream, rowlist, count);
    else if (nrows > 0)
        hipLaunchKernelGGL(build_row_caches_wave<4>, dim3(g), dim3(64 * CBW), 0, stream, n, ld, cost, v, cache_col, cache_val, rowmap, same,
                           cp.stream, rowlist, count);
    // (runs of identical rows: one cache per run, copied to the rest)
    if (same)
        hipLaunchKernelGGL(replicate_group_caches, dim3(std::max(1, std::min((n + 3) / 4, 2048))), dim3(256), 0, stream, n, same, cache_col,
                           cache_val);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

template <int CH, bool LDS_STATE>
static int launch_batch(const F32Plan &pl, std::vector<F32Job> &jobs, hipStream_t stream, hipEvent_t ev_cache_done,
                        hipEvent_t ev_arr_done, DevBuf &d_c2, DevBuf &d_la) {
    const int n = pl.n;
    std::vector<int> live;
    for (int b = 0; b < (int)jobs.size(); b++) if (jobs[b].alive()) live.push_back(b);
    const int nl = (int)live.size();
    if (!nl) return CYTO_OK;
    int rc;
    const bool cs_lds = !LDS_STATE && n <= 65535 && !pl.no_cs_lds;
    void (*kern)(const Chain2Args *) = jv_chain2<CH, LDS_STATE, false>;
    if constexpr (!LDS_STATE) { if (cs_lds) kern = jv_chain2<CH, false, true>; }
    auto build_all_caches = [&]() -> int {
        for (int b : live) {
            const Chain2Args &a = jobs[b].c2;
            const int r2 = build_caches(pl.cache, n, a.ld, a.cost, a.rowmap, a.fws, a.cache_col, a.cache_val, jobs[b].same(n), stream);
            if (r2) return r2;
        }
        return CYTO_OK;
    };
    // argument blocks of the batch, in `live` order
    std::vector<Chain2Args> h_c2((size_t)nl);
    std::vector<LazyArgs> h_la((size_t)nl);
    size_t shm_aug = 0, shm_lazy = 0;
    for (int k = 0; k < nl; k++) {
        F32Job &j = jobs[live[k]];
        h_c2[k] = j.c2; h_la[k] = j.la;
        if (!LDS_STATE) h_la[k].may_bail = 0;                        // only the dense jv_aug2<CH, true> can take over
        shm_aug = std::max(shm_aug, j.shm_aug); shm_lazy = std::max(shm_lazy, j.shm_lazy);
    }
    if ((rc = d_c2.alloc(sizeof(Chain2Args) * nl, stream)) || (rc = d_la.alloc(sizeof(LazyArgs) * nl, stream))) return rc;
    CYTO_HIP(hipMemcpyAsync(d_c2.p, h_c2.data(), sizeof(Chain2Args) * nl, hipMemcpyHostToDevice, stream));
    CYTO_HIP(hipMemcpyAsync(d_la.p, h_la.data(), sizeof(LazyArgs) * nl, hipMemcpyHostToDevice, stream));

    if ((rc = build_all_caches())) return rc;
    CYTO_HIP(hipEventRecord(ev_cache_done, stream));
    if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(kern)))) return rc;
    if (pl.shm_chain > (size_t)LDS_DYNAMIC_MAX || shm_aug > (size_t)LDS_DYNAMIC_MAX || shm_lazy > (size_t)LDS_DYNAMIC_MAX) return CYTO_ERR_INTERNAL;
    hipLaunchKernelGGL(kern, dim3(nl), dim3(BLOCK2), pl.shm_chain, stream, d_c2.as<Chain2Args>());
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
    if (!pl.lazy) return launch_dense(d_c2.as<Chain2Args>(), nl);

    // fresh caches (floors against the prices the augmentation starts from), then the cache-certified search
    if ((rc = build_all_caches())) return rc;
    void (*lk)(const LazyArgs *) = pl.lz_lds_state ? jv_aug_lazy<true> : (pl.lz_cs_lds ? jv_aug_lazy<false, true> : jv_aug_lazy<false>);
    if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(lk)))) return rc;
    hipLaunchKernelGGL(lk, dim3(nl), dim3(BLOCK2), shm_lazy, stream, d_la.as<LazyArgs>());
    CYTO_HIP(hipGetLastError());
    if constexpr (LDS_STATE) {
        // which searches gave up?
        constexpr size_t h0 = offsetof(LapStatus, numfree), h1 = offsetof(LapStatus, lazy_done) + sizeof(int);
        bool any_bail = false;
        for (int k = 0; k < nl; k++) any_bail |= h_la[k].may_bail != 0;
        if (any_bail) {
            for (int k = 0; k < nl; k++)
                CYTO_HIP(hipMemcpyAsync(reinterpret_cast<char *>(&jobs[live[k]].h_hand) + h0, jobs[live[k]].c2.misc + h0, h1 - h0, hipMemcpyDeviceToHost,
                                        stream));
            CYTO_HIP(hipStreamSynchronize(stream));
            std::vector<Chain2Args> cont;
            for (int k = 0; k < nl; k++) {
                const F32Job &j = jobs[live[k]];
                if (h_la[k].may_bail && j.h_hand.lazy_done < j.h_hand.numfree) { Chain2Args a = h_c2[k]; a.aug_start = j.h_hand.lazy_done; cont.push_back(a); }
            }
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

// the counters every solver keeps, as cyto_lap_info reports them
void info_from_counters(cyto_lap_info *info, int n, const LapStatus &h) {
    info->scans_colred = n;
    info->scans_redtransfer = h.counters[C_RT];
    info->scans_arr = h.counters[C_ARR];
    info->scans_aug_init = h.counters[C_AUG_INIT];
    info->scans_aug_relax = h.counters[C_AUG_RELAX];
    info->augmentations = h.counters[C_AUGS];
    info->path_hops = h.counters[C_HOPS];
    info->free_after_colred = h.counters[C_FREE_CR];
    info->free_after_arr1 = h.counters[C_FREE_A1];
    info->free_after_arr2 = h.counters[C_FREE_A2];
}

// All problems have the same n.  jobs[b].status carries per-problem failures (non-finite costs, solver status); the
// return value reports failures of the batch as a whole (allocation, HIP).
static int lap_solve_f32_batch(int n, std::vector<F32Job> &jobs, int device_id, hipStream_t stream, const cyto_lap_opts &opts) {
    const int nb = (int)jobs.size();
    if (nb == 0) return CYTO_OK;
    if (n <= 0) return CYTO_ERR_BAD_ARG;
    if (n > FAST_NMAX) return CYTO_ERR_UNSUPPORTED;
    int rc = check_opts(opts);
    if (rc) return rc;
    if ((rc = select_device(device_id))) return rc;
    Events<6> ev;                                   // destroyed on every return path
    if ((rc = ev.create())) return rc;
    const hipEvent_t e0 = ev[0], e1 = ev[1], e1b = ev[2], e1c = ev[3], e1d = ev[4], e2 = ev[5];

    F32Plan pl;
    pl.n = n;
    pl.colblocks = (n + 256 * 4 - 1) / (256 * 4);
    pl.rowblocks = (2048 + pl.colblocks - 1) / pl.colblocks;
    pl.rowblocks = max(1, min(pl.rowblocks, (n + 15) / 16));
    pl.rows_per_block = (n + pl.rowblocks - 1) / pl.rowblocks;
    pl.rowblocks = (n + pl.rows_per_block - 1) / pl.rows_per_block;
    // (measured, tools/cache_build_bench.py, gpurun_out/r04v: n = 20 000: 8 waves per CU x 8 quads in flight 0.404 ms = 3.96 TB/s, 50 000:
    //  2.13 ms = 4.69 TB/s -- the workgroup-per-row builders 0.750 / 3.27 ms; n = 10 000: 32 x 4 0.126 ms, 8 x 8 0.137, old 0.183:
    //  with few rows per wave the second sweep of a wave's first row, from L2, costs less than the waves it would take away)
    //  A few-cell-type matrix (tools/cache_build_bench.py 20000 --typed, gpurun_out/r04x) is another matter: its rows sit at different
    //  levels, a neighbour's floor fits 6 % of them, nearly every row is swept twice (the second time from L2 by its one wave) and what
    //  counts is how many waves there are: 8 x 8 1.36 ms, 20 x 8 1.01 ms, 32 x 4 1.02 ms, old 0.97 ms.  20 waves x 8 quads is within
    //  5 % of the best setting of every instance measured (uniform 20 000: 0.412 ms, 50 000: 2.25 ms, 10 000: 0.123 ms).
    //  n = 50 000 prefers 8 waves per CU by more than the build's own time (same box, gpurun_out/r04z: row reduction 21.5-23.0 ms after a
    //  build with 8 waves, 24.0-24.8 ms after one with 20 -- 183 instead of 146 full-row bids, each holding up a round for one 200-KB sweep).
    pl.cache.unroll = 8;
    pl.cache.waves = n > 32768 ? 8 : 20;
    // (cyto_lap_opts.cache_waves / cache_unroll / cache_stream -- tools/cache_build_bench.py and the builder tests; cache_waves = -1,
    //  which selected the round-3 builders, is the default now)
    if (opts.cache_waves > 0) pl.cache.waves = opts.cache_waves;
    if (opts.cache_unroll != 0) pl.cache.unroll = opts.cache_unroll;
    if (opts.cache_stream != 0) pl.cache.stream = opts.cache_stream > 0 ? 1 : 0;
    pl.cache.cus = device_cus(device_id);
    const int per2 = 4 * BLOCK2;
    // which chain variant: by size, or the large-n variants forced at a small n (opts.chain_variant; the test-suite
    // runs them on instances the CPU oracle solves in a second)
    // which solver: the wide one (lap_wide.hip) unless the caller selected the chain solver or one of its kernels explicitly.
    // A batch runs its problems side by side, a workgroup each, through either
    const bool chain_opts = opts.chain_variant || opts.augmentation || opts.no_handover || opts.inject_exceptions ||
                            opts.group_state_global || opts.aux_state_global;
    pl.wide = opts.mode == 2 || (opts.mode == 0 && !chain_opts);
    pl.force_l2 = opts.chain_variant != 0;
    pl.no_cs_lds = opts.chain_variant == 3;            // (3: as 2, with colsol in global memory too -- what n > 65 535 uses)
    pl.lds_variant = !pl.force_l2 && n <= 13 * per2;
    // cache-certified augmentation: the default above 5120 columns (measured cross-over with the register-resident dense
    // search on uniform and duplicated-row instances), the only one beyond 26 624
    pl.lazy = opts.augmentation == 2 || !pl.lds_variant || (opts.augmentation == 0 && n > 5120);
    const int npad = (n + 3) & ~3;
    const size_t npad6 = (((size_t)npad * 6) + 15) & ~(size_t)15, npad2 = (((size_t)npad * 2) + 15) & ~(size_t)15;
    const size_t nb24 = (size_t)((((n + 63) / 64) + 511) & ~511) * 8 + (size_t)((n + 63) / 64) * 24 + 16;
    const size_t lds_budget = LDS_DYNAMIC_MAX;
    pl.lz_lds_state = n <= 65535 && !pl.force_l2 && npad6 + nb24 <= lds_budget;
    pl.lz_cs_lds = !pl.lz_lds_state && n <= 65535 && !pl.no_cs_lds && npad2 + nb24 <= lds_budget;
    pl.lz_base_shm = (pl.lz_lds_state ? npad6 : (pl.lz_cs_lds ? npad2 : 0)) + nb24;
    const bool cs_lds_chain = !pl.lds_variant && n <= 65535 && !pl.no_cs_lds;
    pl.shm_chain = pl.lds_variant ? (((size_t)npad * 6 + 15) / 16) * 16 : (cs_lds_chain ? (((size_t)npad * 2 + 15) / 16) * 16 : 16);

    const size_t nT = (size_t)n * sizeof(float), nI = (size_t)n * sizeof(int32_t);
    // First caches from the column reduction's pass (fused_*, above): one float32 problem per call on the wide solver, no row map, the
    // streaming builder's contract (cache_stream != -1), from 32 768 rows on.  A few-cell-type matrix gives the lists up (its sampled
    // minima lie far above the final ones) and has paid the sample and the appends for nothing: 27.29 -> 27.72 ms at 20 000^2, more
    // than that leg's spread, so the gate starts above it.
    // (developer knob, read once per process: CYTO_CACHE_FUSED = 1 or unset: as above; 0: never; 2: from 2 048 rows on -- the tests)
    const int fused_knob = CYTO_KNOB("CYTO_CACHE_FUSED").set ? CYTO_KNOB("CYTO_CACHE_FUSED").value : 1;
    const bool fused_gate = fused_knob != 0 && nb == 1 && pl.wide && !jobs[0].rowmap_host && pl.cache.stream == 1 &&
                            n >= (fused_knob >= 2 ? FUSED_S : 32768);
    const int fused_rs = std::min(1024, n / 2);                   // rows sampled for w
    // ---- stage 1 (every problem, back to back on the stream: full-chip streaming kernels): column reduction, row groups ----
    CYTO_HIP(hipEventRecord(e0, stream));
    for (F32Job &j : jobs) {
        if (!j.cost || j.ld < n) { j.status = CYTO_ERR_BAD_ARG; continue; }
        // optional row map: validated on the host (non-decreasing: duplicated spot rows are contiguous, as np.repeat makes
        // them), the distinct rows in use and the first LAP row of each go to the device with it
        const int nstored = j.rowmap_host ? j.nu : n;
        std::vector<int32_t> ulist, ufirst;
        if (j.rowmap_host) {
            if (j.nu <= 0) { j.status = CYTO_ERR_BAD_ARG; continue; }
            bool ok = true;
            for (int i = 0; i < n && ok; i++) {
                const int32_t r = j.rowmap_host[i];
                ok = r >= 0 && r < j.nu && (i == 0 || r >= j.rowmap_host[i - 1]);
                if (ok && (i == 0 || r != j.rowmap_host[i - 1])) { ulist.push_back(r); ufirst.push_back(i); }
            }
            if (!ok) { j.status = CYTO_ERR_BAD_ARG; continue; }
            j.nused = (int)ulist.size();
        }
        // the kernels want 16-byte aligned rows: pitch a multiple of 4 elements
        j.dcost = j.cost; j.dld = j.ld;
        const bool aligned = j.cost_on_device && (j.ld % 4 == 0) && ((reinterpret_cast<uintptr_t>(j.cost) & 15) == 0);
        if (!aligned) {
            j.dld = ((int64_t)n + 3) / 4 * 4;
            if ((rc = j.staged.alloc((size_t)nstored * j.dld * sizeof(float), stream))) return rc;
            CYTO_HIP(hipMemcpy2DAsync(j.staged.p, j.dld * sizeof(float), j.cost, j.ld * sizeof(float), (size_t)n * sizeof(float), nstored,
                                      j.cost_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
            j.dcost = j.staged.as<float>();
        }
        if (j.rowmap_host) {
            if ((rc = j.b_rowmap.alloc(nI, stream)) || (rc = j.b_ulist.alloc((size_t)j.nused * 4, stream)) || (rc = j.b_ufirst.alloc((size_t)j.nused * 4, stream)))
                return rc;
            CYTO_HIP(hipMemcpyAsync(j.b_rowmap.p, j.rowmap_host, nI, hipMemcpyHostToDevice, stream));
            CYTO_HIP(hipMemcpyAsync(j.b_ulist.p, ulist.data(), (size_t)j.nused * 4, hipMemcpyHostToDevice, stream));
            CYTO_HIP(hipMemcpyAsync(j.b_ufirst.p, ufirst.data(), (size_t)j.nused * 4, hipMemcpyHostToDevice, stream));
            CYTO_HIP(hipStreamSynchronize(stream));       // ulist / ufirst are locals
        }
        // workspace (blocks of the device cache: no hipMalloc / hipFree once a size has been seen).  The candidate lists are the one
        // large part (n x 4 KB: 205 MB at n = 50 000): where the block with them cannot be had, the solve runs without them
        j.fused = fused_gate;
        for (;;) {
            size_t off = 0;
            auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
            const size_t o_fws = take(6 * nT + 64), o_iws = take(10 * nI + 64), o_imin = take(nI), o_pmin = take((size_t)pl.rowblocks * nT),
                         o_parg = take((size_t)pl.rowblocks * nI), o_misc = take(sizeof(LapStatus)), o_same = take(nI), o_gid = take(nI),
                         o_ccol = take((size_t)n * KC * sizeof(uint32_t)), o_cval = take((size_t)n * KC * sizeof(float));
            const size_t o_fw = j.fused ? take(nT + 16) : 0, o_fth = j.fused ? take(nT) : 0, o_fcnt = j.fused ? take(nI + 256) : 0,
                         o_frows = j.fused ? take(nI) : 0, o_flist = j.fused ? take((size_t)n * COLRED_CAP * sizeof(uint2)) : 0;
            rc = j.slab.alloc(off, stream);
            if (rc == CYTO_ERR_NOMEM && j.fused) { (void)hipGetLastError(); j.fused = false; continue; }      // (the failed hipMalloc's error is not the solve's)
            if (rc) return rc;
            char *base = j.slab.as<char>();
            if (j.fused) {
                j.f_w = reinterpret_cast<float *>(base + o_fw); j.f_theta = reinterpret_cast<float *>(base + o_fth);
                j.f_cnt = reinterpret_cast<int32_t *>(base + o_fcnt); j.f_nfail = j.f_cnt + n;      // (one memset clears both)
                j.f_rows = reinterpret_cast<int32_t *>(base + o_frows); j.f_list = reinterpret_cast<uint2 *>(base + o_flist);
            }
            j.b_fws.view(base + o_fws, stream); j.b_iws.view(base + o_iws, stream); j.b_imin.view(base + o_imin, stream);
            j.b_pmin.view(base + o_pmin, stream); j.b_parg.view(base + o_parg, stream); j.b_misc.view(base + o_misc, stream);
            j.b_same.view(base + o_same, stream); j.b_gid.view(base + o_gid, stream); j.b_ccol.view(base + o_ccol, stream);
            j.b_cval.view(base + o_cval, stream);
            break;
        }
        // float workspace: v | u | ... ; int workspace: rowsol | colsol | matches | freerows | rtrows | pred | ...
        float *d_v = j.b_fws.as<float>();
        int32_t *d_rowsol = j.b_iws.as<int32_t>(), *d_colsol = d_rowsol + n, *d_matches = d_rowsol + 2 * (size_t)n;
        CYTO_HIP(hipMemsetAsync(j.b_misc.p, 0, sizeof(LapStatus), stream));
        CYTO_HIP(hipMemsetAsync(d_rowsol, 0xFF, nI, stream));
        CYTO_HIP(hipMemsetAsync(d_matches, 0, nI, stream));
        {   // the column minima need every DISTINCT row once: with a row map only the stored rows in use are swept
            const int nrows = j.rowmap_host ? j.nused : n;
            const int rpb = j.rowmap_host ? (nrows + pl.rowblocks - 1) / pl.rowblocks : pl.rows_per_block;
            const int rblocks = j.rowmap_host ? (nrows + rpb - 1) / rpb : pl.rowblocks;
            if (j.fused) {
                // w from the first rows (the partial minima go through pmin / parg, which the full pass then overwrites), theta, and
                // the full pass with appends
                const int srb0 = std::max(1, std::min(pl.rowblocks, (fused_rs + 15) / 16)), srpb = (fused_rs + srb0 - 1) / srb0,
                          srb = (fused_rs + srpb - 1) / srpb;
                hipLaunchKernelGGL(colred_partial<float>, dim3(pl.colblocks, srb), dim3(256), 0, stream, n, j.dld, j.dcost, srpb,
                                   j.b_pmin.as<float>(), j.b_parg.as<int32_t>(), &j.st()->nonfinite, fused_rs, (const int32_t *)nullptr,
                                   (const int32_t *)nullptr);
                hipLaunchKernelGGL(fused_w, dim3((n + 255) / 256), dim3(256), 0, stream, n, srb, j.b_pmin.as<float>(), j.f_w);
                hipLaunchKernelGGL(fused_theta, dim3((n + 3) / 4), dim3(256), 0, stream, n, j.dld, j.dcost, j.f_w, j.f_theta);
                CYTO_HIP(hipMemsetAsync(j.f_cnt, 0, nI + sizeof(int32_t), stream));
                const ColredAppend ap = {j.f_w, j.f_theta, j.f_cnt, j.f_list};
                hipLaunchKernelGGL(colred_partial_append, dim3(pl.colblocks, rblocks), dim3(256), 0, stream, n, j.dld, j.dcost, rpb,
                                   j.b_pmin.as<float>(), j.b_parg.as<int32_t>(), &j.st()->nonfinite, nrows, ap);
            } else
            hipLaunchKernelGGL(colred_partial<float>, dim3(pl.colblocks, rblocks), dim3(256), 0, stream, n, j.dld, j.dcost, rpb,
                               j.b_pmin.as<float>(), j.b_parg.as<int32_t>(), &j.st()->nonfinite, nrows,
                               j.rowmap_host ? j.b_ulist.as<int32_t>() : (const int32_t *)nullptr,
                               j.rowmap_host ? j.b_ufirst.as<int32_t>() : (const int32_t *)nullptr);
            hipLaunchKernelGGL(colred_finish<float>, dim3((n + 255) / 256), dim3(256), 0, stream, n, rblocks, j.b_pmin.as<float>(),
                               j.b_parg.as<int32_t>(), d_v, j.b_imin.as<int32_t>(), d_rowsol, d_matches);
        }
        launch_colred_assign(n, j.b_imin.as<int32_t>(), d_rowsol, d_colsol, stream);
    }
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipEventRecord(e1, stream));
    // duplicate-row groups: runs of bitwise identical consecutive rows
    const bool want_groups = n >= 2;
    for (F32Job &j : jobs) {
        if (!j.alive()) continue;
        j.h_ngroups = n;
        if (want_groups) {
            if (j.rowmap_host)
                hipLaunchKernelGGL(rows_same_from_map, dim3((n + 255) / 256), dim3(256), 0, stream, n, j.b_rowmap.as<int32_t>(), j.b_same.as<int32_t>());
            else
                hipLaunchKernelGGL(rows_same_as_prev<float>, dim3(min(n, 2048)), dim3(256), 0, stream, n, j.dld, j.dcost, j.b_same.as<int32_t>());
            hipLaunchKernelGGL(rows_group_ids, dim3(1), dim3(1024), 0, stream, n, j.b_same.as<int32_t>(), j.b_gid.as<int32_t>(),
                               &j.st()->ngroups);
        }
        if (j.fused) {                                             // the lists against the final prices; what fails goes on f_rows
            hipLaunchKernelGGL(fused_fixup, dim3((n + 3) / 4), dim3(256), 0, stream, n, j.b_fws.as<float>(), j.f_theta, j.f_cnt, j.f_list,
                               j.b_same.as<int32_t>(), j.b_ccol.as<uint32_t>(), j.b_cval.as<float>(), j.f_rows, j.f_nfail, fused_min_kept(n));
            CYTO_HIP(hipMemcpyAsync(&j.h_fused_failed, j.f_nfail, sizeof(int), hipMemcpyDeviceToHost, stream));
        }
        // a non-finite cost makes every later comparison meaningless: that problem stops before the chain
        CYTO_HIP(hipMemcpyAsync(&j.h_nonfinite, &j.st()->nonfinite, sizeof(int), hipMemcpyDeviceToHost, stream));
        if (want_groups) CYTO_HIP(hipMemcpyAsync(&j.h_ngroups, &j.st()->ngroups, sizeof(int), hipMemcpyDeviceToHost, stream));
    }
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipStreamSynchronize(stream));
    CYTO_HIP(hipEventRecord(e1b, stream));

    // ---- stage 2: per-problem argument blocks of the chain solver ----
    for (F32Job &j : jobs) {
        if (!j.alive()) continue;
        if (j.h_nonfinite) { j.status = CYTO_ERR_NONFINITE; continue; }
        if (pl.wide) continue;
        float *d_v = j.b_fws.as<float>(), *d_u = d_v + n;
        int32_t *d_rowsol = j.b_iws.as<int32_t>(), *d_colsol = d_rowsol + n, *d_free = d_rowsol + 3 * (size_t)n;
        const int ng = j.h_ngroups;
        Chain2Args &c2 = j.c2;
        c2.n = n; c2.ld = j.dld; c2.cost = j.dcost; c2.fws = d_v; c2.iws = d_rowsol;
        c2.cache_col = j.b_ccol.as<uint32_t>(); c2.cache_val = j.b_cval.as<float>(); c2.misc = j.b_misc.as<char>();
        // duplicate-row skip: per-group state in LDS when it fits beside v (4 B) and colsol (2 B) per column
        c2.rowgid = j.b_gid.as<int32_t>(); c2.ngroups = ng; c2.gmode = 0; c2.g_hbest = nullptr; c2.g_hstamp = nullptr;
        c2.auxlds = 0; c2.aug_start = 0;
        c2.rowmap = j.rowmap();
        LazyArgs &la = j.la;
        memset(&la, 0, sizeof la);
        j.shm_lazy = pl.lz_base_shm;
        if (pl.lazy) {
            la.n = n; la.ld = j.dld; la.cost = j.dcost; la.gv = d_v; la.gu = d_u; la.sumvd = d_v + 2 * (int64_t)n;
            la.cassign = d_v + 3 * (int64_t)n; la.dkey = reinterpret_cast<uint64_t *>(d_v + 4 * (int64_t)n);
            la.rowsol = d_rowsol; la.colsol = d_colsol; la.freerows = d_free;
            la.srow = d_rowsol + 6 * (int64_t)n;      // [n+1]: runs into the next slot, which the lazy path does not use
            la.slist = d_rowsol + 8 * (int64_t)n; la.slevel = d_rowsol + 9 * (int64_t)n;
            la.rowgid = j.b_gid.as<int32_t>(); la.cache_col = j.b_ccol.as<uint32_t>(); la.cache_val = j.b_cval.as<float>();
            la.rowmap = j.rowmap();
            la.misc = j.b_misc.as<char>(); la.ngroups = ng; la.gmode = 0; la.g_hbest = nullptr; la.g_hstamp = nullptr;
            la.may_bail = opts.no_handover ? 0 : 1;   // (launch_batch clears it where no dense kernel can take over)
            la.debug_exc = opts.inject_exceptions;
            if (want_groups && ng < n) {
                if (!opts.group_state_global && j.shm_lazy + (size_t)ng * 8 <= lds_budget) { la.gmode = 1; j.shm_lazy += (size_t)ng * 8; }
                else {
                    la.gmode = 2;
                    if ((rc = j.b_lzhb.alloc((size_t)ng * 4, stream)) || (rc = j.b_lzhs.alloc((size_t)ng * 4, stream))) return rc;
                    CYTO_HIP(hipMemsetAsync(j.b_lzhs.p, 0, (size_t)ng * 4, stream));
                    la.g_hbest = j.b_lzhb.as<float>(); la.g_hstamp = j.b_lzhs.as<int32_t>();
                }
            }
        }
        if (want_groups && ng < n) {
            // LDS beside the group state: v (4 B) + colsol (2 B) per column on the LDS-resident path
            const size_t lds_state = pl.lds_variant ? (size_t)npad * 6 : (size_t)((n + 31) / 32) * 4;
            if (!opts.group_state_global && lds_state + (size_t)ng * 8 + 8192 <= 160 * 1024) c2.gmode = 1;
            else {
                c2.gmode = 2;
                if ((rc = j.b_ghb.alloc((size_t)ng * 4, stream)) || (rc = j.b_ghs.alloc((size_t)ng * 4, stream))) return rc;
                CYTO_HIP(hipMemsetAsync(j.b_ghs.p, 0, (size_t)ng * 4, stream));
                c2.g_hbest = j.b_ghb.as<float>(); c2.g_hstamp = j.b_ghs.as<int32_t>();
            }
        }
        // dense augmentation: its LDS (prices, colsol, per-group state, and the per-column auxiliaries when they fit)
        const size_t base_aug = (((pl.lds_variant ? (size_t)npad * 6 : 0) + (c2.gmode == 1 ? (size_t)ng * 8 : 0) + 15) / 16) * 16;
        c2.auxlds = (!opts.aux_state_global && pl.lds_variant && ng < 65536 && base_aug + (size_t)npad * 6 + 4096 <= 160 * 1024) ? 1 : 0;
        j.shm_aug = base_aug + (c2.auxlds ? (size_t)npad * 6 : 0) + 32;
    }

    // ---- stage 3: the solver, one launch per phase for the whole batch ----
    DevBuf d_c2, d_la;
    if (pl.wide) {
        const WidePlan wp = {n, opts.wide_rounds < 0 ? 0 : (opts.wide_rounds > 0 ? opts.wide_rounds : 4096 + (long long)n / 4),
                             opts.wide_rebuild, opts.wide_wipe, opts.wide_par, pl.cache};
        std::vector<WideJob> wj;
        for (F32Job &j : jobs)
            if (j.alive())
                wj.push_back({j.dcost, j.dld, j.rowmap(), j.b_fws.as<float>(), j.b_iws.as<int32_t>(), j.b_ccol.as<uint32_t>(),
                              j.b_cval.as<float>(), j.b_misc.as<char>(), j.same(n), j.h_ngroups, &j.b_wide});
        if (jobs[0].fused && !wj.empty()) {
            // few enough rows failed: the row builder takes those alone; otherwise (a few-cell-type matrix: the sampled minima lie too
            // far above the final ones) it builds every row as if there had been no lists
            F32Job &j = jobs[0];
            if (j.h_fused_failed <= n / 8) { wj[0].first_rows = j.f_rows; wj[0].first_count = j.h_fused_failed; }
            else j.h_fused_failed = n;
            g_fused_solves.fetch_add(1);
            g_fused_fallback_rows.fetch_add(j.h_fused_failed);
        }
        rc = wide_solve_batch(wp, wj, stream, e1c, e1d);
    } else if (opts.chain_variant >= 2) rc = launch_batch<0, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (pl.force_l2 && n <= 5 * per2) rc = launch_batch<5, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (pl.force_l2 && n <= 16 * per2) rc = launch_batch<16, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (pl.force_l2) rc = launch_batch<0, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (n <= 2 * per2) rc = launch_batch<2, true>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (n <= 5 * per2) rc = launch_batch<5, true>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (n <= 10 * per2) rc = launch_batch<10, true>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (n <= 13 * per2) rc = launch_batch<13, true>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else if (n <= 16 * per2) rc = launch_batch<16, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);
    else rc = launch_batch<0, false>(pl, jobs, stream, e1c, e1d, d_c2, d_la);   // streaming dense refresh, any n
    if (rc) return rc;
    CYTO_HIP(hipEventRecord(e2, stream));
    CYTO_HIP(hipStreamSynchronize(stream));

    // ---- results ----
    float ms_colred = 0, ms_cache = 0, ms_chain = 0, ms_arr = 0, ms_aug = 0;
    bool any_alive = false;
    for (const F32Job &j : jobs) any_alive |= j.alive();
    (void)hipEventElapsedTime(&ms_colred, e0, e1);
    if (any_alive) {
        (void)hipEventElapsedTime(&ms_cache, e1b, e1c); (void)hipEventElapsedTime(&ms_chain, e1c, e2);
        (void)hipEventElapsedTime(&ms_arr, e1c, e1d); (void)hipEventElapsedTime(&ms_aug, e1d, e2);
    }
    for (F32Job &j : jobs) {
        if (!j.alive()) continue;
        LapStatus h;
        int32_t *d_rowsol = j.b_iws.as<int32_t>();
        float *d_v = j.b_fws.as<float>();
        CYTO_HIP(hipMemcpy(&h, j.st(), sizeof h, hipMemcpyDeviceToHost));
        double h_gap[3] = {-1.0, -1.0, -1.0};
        ExactRun ex;
        if (((opts.certify && j.info) || opts.exact) && !h.status) {
            // the float64 certificate (lap_exact.hip): one more streaming pass, on the stream, behind the solve
            DevBuf b_viol;
            if ((rc = b_viol.alloc(((size_t)n + 4) * sizeof(double), stream))) return rc;
            const int g = std::max(1, std::min((n + 3) / 4, pl.cache.cus * 8));
            if ((rc = certify_launch(n, j.dld, j.dcost, j.rowmap(), d_rowsol, d_v, b_viol.as<double>(), g, stream))) return rc;
            // the exact option: the near-tight edges right behind it (the kernel reads the gap on the device)
            const ExactView xv = {j.dcost, j.dld, j.rowmap(), d_rowsol, d_v, j.st()};
            if (opts.exact && (rc = exact_emit(ex, n, opts.exact == 1 ? EXACT_SLOTS_DEFAULT : opts.exact, xv, b_viol.as<double>() + n, g, stream)))
                return rc;
            CYTO_HIP(hipMemcpyAsync(h_gap, b_viol.as<double>() + n, sizeof h_gap, hipMemcpyDeviceToHost, stream));
            CYTO_HIP(hipStreamSynchronize(stream));
            if (opts.exact && (rc = exact_repair(ex, n, xv, h_gap[0], g, stream))) return rc;
        }
        if (j.rowsol) CYTO_HIP(hipMemcpy(j.rowsol, d_rowsol, nI, hipMemcpyDeviceToHost));
        if (j.colsol) CYTO_HIP(hipMemcpy(j.colsol, d_rowsol + n, nI, hipMemcpyDeviceToHost));
        if (j.u) CYTO_HIP(hipMemcpy(j.u, d_v + n, nT, hipMemcpyDeviceToHost));
        if (j.v) CYTO_HIP(hipMemcpy(j.v, d_v, nT, hipMemcpyDeviceToHost));
        if (j.total) CYTO_HIP(hipMemcpy(j.total, &j.st()->total, sizeof(double), hipMemcpyDeviceToHost));   // (exact_repair rewrites it)
        if (j.info) {
            cyto_lap_info *info = j.info;
            memset(info, 0, sizeof *info);
            // (kernel times of a batch are those of the whole batch: its problems share every launch)
            info->ms_colred = ms_colred; info->ms_cache = ms_cache; info->ms_chain = ms_chain; info->ms_arr = ms_arr; info->ms_aug = ms_aug;
            info->ms_total = info->ms_colred + info->ms_cache + info->ms_chain;
            info_from_counters(info, n, h);
            info->hbm_row_reads = (j.fused ? (int64_t)n + fused_rs + j.h_fused_failed : 2 * (int64_t)n) + h.counters[C_ROWS_READ];
            info->dense_refreshes = h.counters[C2_DENSE_REFRESH];
            info->aug_scans_skipped = h.counters[C2_AUG_SKIPPED];
            info->aug_dense_scans = h.counters[C2_AUG_DENSE];
            info->aug_sparse_inits = h.counters[C2_AUG_SPARSE_INIT];
            info->aug_handover = (pl.lazy && !pl.wide && h.lazy_done < h.numfree) ? h.lazy_done : -1;
            info->row_groups = j.h_ngroups;
            info->certified = h_gap[0] >= 0.0 ? 1 : 0;
            info->gap_f64 = h_gap[0] >= 0.0 ? h_gap[0] : 0.0; info->gap_max_f64 = h_gap[0] >= 0.0 ? h_gap[1] : 0.0;
            info->gap_rows = h_gap[0] >= 0.0 ? (int64_t)h_gap[2] : 0;
            info->exact_status = ex.status; info->exact_edges = ex.edges; info->exact_free_rows = ex.free_rows;
            info->exact_changed_rows = ex.changed; info->exact_overflow_rows = ex.overflow;
            info->exact_ms_emit = ex.ms_emit; info->exact_ms_repair = ex.ms_repair;
            if (pl.wide) {
                const long long *wc = h.wide, *tm = h.timers;       // (timers: diagnostics for tools/wide_large.py; 100 MHz ticks)
                info->wide = 1;
                info->wide_rounds = wc[WC_ROUNDS]; info->wide_retired = wc[WC_RETIRED]; info->wide_dense_arr = wc[WC_DENSE_ARR];
                info->wide_dense_aug = wc[WC_DENSE_AUG]; info->wide_aug_rounds = wc[WC_AUG_ROUNDS]; info->wide_aug_settled = wc[WC_AUG_PROCESSED];
                info->wide_trivial = wc[WC_TRIVIAL]; info->wide_verify_passes = wc[WC_VERIFY_PASSES]; info->wide_aug_launches = wc[WC_AUG_LAUNCHES];
                info->wide_list_rounds = tm[WT_LIST_ROUNDS]; info->wide_chain_rounds = tm[WT_CHAIN_ROUNDS];
                info->wide_ms_list = tm[WT_LIST_TICKS] * 1e-5; info->wide_ms_chain = tm[WT_CHAIN_TICKS] * 1e-5;
                info->wide_ms_aug_rounds = tm[WT_AUG_ROUNDS_TICKS] * 1e-5; info->wide_ms_aug_verify = tm[WT_AUG_VERIFY_TICKS] * 1e-5;
                info->wide_ms_aug_finish = tm[WT_AUG_FINISH_TICKS] * 1e-5; info->wide_ms_aug_trivial = tm[WT_AUG_TRIVIAL_TICKS] * 1e-5;
                info->wide_arr_launches = tm[WT_ARR_LAUNCHES]; info->wide_scaled = tm[WT_SCALED]; info->wide_phases = tm[WT_PHASES];
                info->wide_par_batches = tm[WT_PAR_BATCHES]; info->wide_par_discarded = tm[WT_PAR_DISCARDED];
            }
        }
        if (h.status) j.status = CYTO_ERR_INTERNAL;
        if (ex.status == 3 && j.alive()) {
            // E over its cap: the float64 polish of this problem (one at a time in a batch: it widens the whole matrix)
            double ms = 0.0;
            const int r2 = lap_polish_f64(n, j.cost, j.ld, j.cost_on_device, j.rowmap_host, j.nu, ex.v.data(), j.rowsol, j.colsol, j.u, j.v,
                                          j.total, &ms, device_id, stream);
            if (r2) j.status = r2;
            if (j.info) { j.info->polished = 1; j.info->polish_ms = ms; }
        }
    }
    return CYTO_OK;
}

// one float32 problem = a batch of one
static int lap_solve_f32_one(int n, const float *cost, int64_t ld, int cost_on_device, const int32_t *rowmap_host, int nu, int32_t *rowsol,
                             int32_t *colsol, float *u, float *v, double *total, cyto_lap_info *info, int device_id, hipStream_t stream,
                             const cyto_lap_opts &opts) {
    if (n <= 0 || !cost || ld < n) return CYTO_ERR_BAD_ARG;
    std::vector<F32Job> jobs(1);
    F32Job &j = jobs[0];
    j.cost = cost; j.ld = ld; j.cost_on_device = cost_on_device; j.rowmap_host = rowmap_host; j.nu = nu;
    cyto_lap_info li = {};
    std::vector<float> v_keep;
    cyto_lap_opts o = opts;
    if (opts.polish) { o.certify = 1; if (!v) { v_keep.resize((size_t)n); v = v_keep.data(); } }
    j.rowsol = rowsol; j.colsol = colsol; j.u = u; j.v = v; j.total = total; j.info = (info || opts.polish) ? &li : nullptr;
    int rc = lap_solve_f32_batch(n, jobs, device_id, stream, o);
    rc = rc ? rc : j.status;
    if (!rc && opts.polish && li.certified && li.gap_f64 > 0.0) {
        double ms = 0.0;
        rc = lap_polish_f64(n, cost, ld, cost_on_device, rowmap_host, nu, v, rowsol, colsol, u, v_keep.empty() ? v : nullptr, total, &ms, device_id, stream);
        li.polished = 1; li.polish_ms = ms;
    }
    if (info && (info != &li)) *info = li;
    return rc;
}
int lap_solve_f32(int n, const float *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                  float *u, float *v, double *total, cyto_lap_info *info, int device_id, hipStream_t stream,
                  const cyto_lap_opts &opts) {
    return lap_solve_f32_one(n, cost, ld, cost_on_device, nullptr, 0, rowsol, colsol, u, v, total, info, device_id, stream, opts);
}

// C ABI helper of cyto_lap_batch_f32 (batch.hip): problems of equal size go through the chains together
int lap_batch_same_n(int n, int nb, const float *const *cost, const int64_t *ld, int cost_on_device, int32_t *const *rowsol,
                     int32_t *const *colsol, float *const *u, float *const *v, double *total, cyto_lap_info *info, int *status,
                     int device_id, hipStream_t stream, const int32_t *const *rowmap, const int *nu, const cyto_lap_opts *opts) {
    std::vector<F32Job> jobs((size_t)nb);
    for (int b = 0; b < nb; b++) {
        F32Job &j = jobs[(size_t)b];
        j.cost = cost[b]; j.ld = ld[b]; j.cost_on_device = cost_on_device;
        if (rowmap && rowmap[b]) { j.rowmap_host = rowmap[b]; j.nu = nu ? nu[b] : 0; }
        j.rowsol = rowsol ? rowsol[b] : nullptr; j.colsol = colsol ? colsol[b] : nullptr;
        j.u = u ? u[b] : nullptr; j.v = v ? v[b] : nullptr;
        j.total = total ? &total[b] : nullptr; j.info = info ? &info[b] : nullptr;
    }
    const int rc = lap_solve_f32_batch(n, jobs, device_id, stream, opts ? *opts : k_default_opts);
    for (int b = 0; b < nb; b++) status[b] = rc ? rc : jobs[(size_t)b].status;
    return rc;
}

// float64 -> float32 of a row-major matrix (the cast numpy's astype(float32) performs: round to nearest even)
__global__ __launch_bounds__(256) void narrow_f64_to_f32(int n, int64_t lds_, const double *__restrict__ src, int64_t ldd,
                                                         float *__restrict__ dst) {
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y)
        for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) dst[row * ldd + c] = (float)src[row * lds_ + c];
}

int narrow_to_f32(int n, int64_t ld_src, const double *src, int64_t ld_dst, float *dst, hipStream_t stream) {
    hipLaunchKernelGGL(narrow_f64_to_f32, matrix_copy_grid(n), dim3(256), 0, stream, n, ld_src, src, ld_dst, dst);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

}  // namespace cyto

extern "C" {

// The call the reference makes, `lapjv(cost_scaled)` with a float64 numpy array solved in float32
// (linear_assignment_solvers.py:38): the matrix goes to the device as it is and is narrowed there, instead of a
// float64 -> float32 pass over 8 n^2 bytes on the host first.
int cyto_lap_f32_from_f64(int n, const double *cost_host, int64_t ld, int32_t *rowsol, int32_t *colsol, float *u, float *v,
                          double *total, cyto_lap_info *info, int device_id, void *stream_) {
    if (n <= 0 || !cost_host || ld < n) return CYTO_ERR_BAD_ARG;
    int rc = cyto::select_device(device_id);
    if (rc) return rc;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int64_t ldd = ((int64_t)n + 3) & ~(int64_t)3;
    cyto::DevBuf d64, d32;
    if ((rc = d64.alloc((size_t)n * n * sizeof(double), stream)) || (rc = d32.alloc((size_t)n * ldd * sizeof(float), stream))) return rc;
    CYTO_HIP(hipMemcpy2DAsync(d64.p, (size_t)n * sizeof(double), cost_host, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n,
                              hipMemcpyHostToDevice, stream));
    if ((rc = cyto::narrow_to_f32(n, (int64_t)n, d64.as<double>(), ldd, d32.as<float>(), stream))) return rc;
    CYTO_HIP(hipStreamSynchronize(stream));
    d64.reset();                                           // the float64 copy is not needed during the solve
    return cyto::lap_solve_f32(n, d32.as<float>(), ldd, 1, rowsol, colsol, u, v, total, info, device_id, stream, cyto::k_default_opts);
}

int cyto_lap_f32(int n, const float *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                 float *u, float *v, double *total, cyto_lap_info *info, int device_id, void *stream) {
    return cyto::lap_solve_f32(n, cost, ld, cost_on_device, rowsol, colsol, u, v, total, info, device_id, reinterpret_cast<hipStream_t>(stream), cyto::k_default_opts);
}

int cyto_lap_f64(int n, const double *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                 double *u, double *v, double *total, cyto_lap_info *info, int device_id, void *stream) {
    return cyto::lap_solve_f64(n, cost, ld, cost_on_device, rowsol, colsol, u, v, total, info, device_id, reinterpret_cast<hipStream_t>(stream), cyto::k_default_opts);
}

int cyto_lap_f32_rowmap(int n, const float *cost_rows, int64_t ld, int nu, int cost_on_device, const int32_t *rowmap,
                        int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total, cyto_lap_info *info, int device_id,
                        void *stream, const cyto_lap_opts *opts) {
    if (n <= 0 || !cost_rows || ld < n || !rowmap || nu <= 0) return CYTO_ERR_BAD_ARG;
    return cyto::lap_solve_f32_one(n, cost_rows, ld, cost_on_device, rowmap, nu, rowsol, colsol, u, v, total, info, device_id,
                                   reinterpret_cast<hipStream_t>(stream), opts ? *opts : cyto::k_default_opts);
}

int cyto_lap_f32_opts(int n, const float *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                      float *u, float *v, double *total, cyto_lap_info *info, int device_id, void *stream, const cyto_lap_opts *opts) {
    return cyto::lap_solve_f32(n, cost, ld, cost_on_device, rowsol, colsol, u, v, total, info, device_id, reinterpret_cast<hipStream_t>(stream), opts ? *opts : cyto::k_default_opts);
}

int cyto_lap_f64_opts(int n, const double *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                      double *u, double *v, double *total, cyto_lap_info *info, int device_id, void *stream, const cyto_lap_opts *opts) {
    return cyto::lap_solve_f64(n, cost, ld, cost_on_device, rowsol, colsol, u, v, total, info, device_id, reinterpret_cast<hipStream_t>(stream), opts ? *opts : cyto::k_default_opts);
}

long long cyto_fused_cache_solves(void) { return cyto::g_fused_solves.load(); }
long long cyto_fused_cache_fallback_rows(void) { return cyto::g_fused_fallback_rows.load(); }

}  // extern "C"
