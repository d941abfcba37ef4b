// lap_jv.hip -- Jonker-Volgenant LAP solver for gfx950 (MI355X), hand-written HIP.
//
// Replaces the reference's single third-party call
//     `_, y, _ = lapjv.lapjv(cost_scaled)`
// (/root/reference/cytospace/linear_assignment_solvers/linear_assignment_solvers.py:34-40).
// Same operand order and the same lowest-index tie-breaking as the CPU oracle (oracle/jv_oracle_impl.h), so rowsol/colsol/u/v
// are bit-identical to it.  This file does two jobs:
//
// (1) The streaming kernels that every float32 solve runs (DESIGN.md section 4.1 has the exactness arguments and the measurements)
//   colred_partial / colred_finish / colred_assign : COLUMN REDUCTION.  The only phase with N^2 independent
//       work: a full-chip streaming pass (float4 per lane, >= 2k workgroups).
//   rows_same_as_prev / rows_group_ids : runs of bitwise identical rows (CytoSPACE repeats every spot row
//       slots[s] times); used to elide provably useless scans in the augmentation.
//   build_row_caches_wave / replicate_group_caches : per row, the <= 63 columns with the smallest reduced cost
//       plus a floor that bounds every other column (a certificate while prices only decrease).
//   colred_partial_append / fused_w / fused_theta / fused_fixup : the first row caches out of the column reduction's own pass.
// (2) The float32 batch driver (lap_solve_f32_batch) and the C entry points.  The driver hands the problems to one of two solvers:
//   the wide solver -- what runs by default -- lap_wide.hip (with lap_wide_rr.hip, lap_wide_drv.hip), or the chain solver (jv_chain2, jv_aug2, jv_aug_lazy), lap_chain_f32.hip.
// The float64 solver (jv_chain<T, CH>, jv_chain_stream) is lap_f64.hip, the float64 certificate and the exact option lap_exact.hip.
//
// Compile with -ffp-contract=off (build.py does): the arithmetic is subtract/compare only,
// but nothing may be re-associated.
#include "cyto_common.h"
#include "lap_dev.h"
#include "lap_chain.h"
#include "lap_chain_f32.h"
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
// scans that provably change nothing (see chain_augment, lap_chain_f32.hip).
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
// Same cache contract as refresh_row (lap_chain_f32.hip: its "v2" comment states the contract).
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
                //  lap_wide_rr.hip, SC_FLOOR_POS) -- the bisection that follows is for rows with ties
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
// -DCYTO_COLRED_PROBE=1 / 2 / 3 (developer builds that only TIME the pass, profiles/r10_headline_leftovers_step0.txt; the driver hands
// every row to the row builder behind them): 1 = no appends at all, the ballots kept; 2 = the atomics kept, no stores; 3 = the stores
// to the positions a count of zero gives, no atomic
#ifndef CYTO_COLRED_PROBE
#define CYTO_COLRED_PROBE 0
#endif
// workgroups of the pass per CU (the plan in cyto_lap_f32_batch; a developer build may set another)
#ifndef CYTO_COLRED_PER_CU
#define CYTO_COLRED_PER_CU 5
#endif
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
#if CYTO_COLRED_PROBE == 1
#pragma unroll
        for (int u = 0; u < RU; u++) asm volatile("" :: "s"(tot[u]));
        (void)my_tot; (void)my_row; (void)old; (void)lt;
#else
#if CYTO_COLRED_PROBE != 3
        if (my_tot) old = (uint32_t)atomicAdd(ap.cnt + my_row, my_tot);
#endif
        asm volatile("" : "+v"(old) :: "memory");                      // (the one wait: the positions and the next group's loads)
#if CYTO_COLRED_PROBE == 2
#pragma unroll
        for (int u = 0; u < RU; u++) asm volatile("" :: "s"(__builtin_amdgcn_readlane((int)old, u)));
        (void)lt;
#else
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
#endif
#endif
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
    DevBuf staged, b_fws, b_iws, b_imin, b_pmin, b_parg, b_misc, b_same, b_gid, b_ccol, b_cval;
    DevBuf b_chain[CHAIN_STATE_BUFS];   // the chain solver's own state (lap_chain_f32.hip allocates it)
    DevBuf b_rowmap, b_ulist, b_ufirst;
    DevBuf b_wide;              // the wide solver's own state (lap_wide_drv.hip allocates it)
    int nused = 0;
    const float *dcost = nullptr; int64_t dld = 0;
    int h_nonfinite = 0, h_ngroups = 0;
    // first caches from the column reduction's pass (fused_*): w | theta | cnt | rowlist | nfail views into the slab, the lists behind them
    bool fused = false; int h_fused_failed = 0;
    float *f_w = nullptr, *f_theta = nullptr; int32_t *f_cnt = nullptr, *f_rows = nullptr, *f_nfail = nullptr; uint2 *f_list = nullptr;
    bool alive() const { return status == CYTO_OK; }
    LapStatus *st() const { return b_misc.as<LapStatus>(); }
    const int32_t *rowmap() const { return rowmap_host ? b_rowmap.as<int32_t>() : nullptr; }
    const int32_t *same(int n) const { return (h_ngroups < n && n >= 2) ? b_same.as<int32_t>() : nullptr; }    // (runs of identical rows)
};

struct F32Plan {            // what depends on n (and the options) only: identical for every problem of the batch
    int n, colblocks, rowblocks, rows_per_block;
    CachePlan cache;
    bool wide;              // the wide solver (lap_wide.hip), not the chain solver (lap_chain_f32.hip)
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
    // which solver: the wide one (lap_wide.hip) unless the caller selected the chain solver or one of its kernels explicitly.
    // A batch runs its problems side by side, a workgroup each, through either
    const bool chain_opts = opts.chain_variant || opts.augmentation || opts.no_handover || opts.inject_exceptions ||
                            opts.group_state_global || opts.aux_state_global;
    pl.wide = opts.mode == 2 || (opts.mode == 0 && !chain_opts);

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
    // The pass with appends waits for a returning atomic per group of four rows, so its time is set by how evenly its waves share the
    // chip, not by how many there are: the plain pass's 2 048 workgroups are 1.34 rounds of this kernel's six waves per SIMD, and the
    // second round runs a third full.  Five workgroups per CU -- one round, every CU alike -- measured best at 50 000^2 (2.26 -> 2.04 ms;
    // six 2.10, four 2.17: profiles/r10_headline_leftovers_step0.txt).  Column minima and the lowest row on ties do not depend on how
    // the rows are dealt to the blocks (colred_finish takes the blocks in row order with a strict comparison).
    if (fused_gate) {
        pl.rowblocks = max(1, min(CYTO_COLRED_PER_CU * pl.cache.cus / pl.colblocks, (n + 15) / 16));
        pl.rows_per_block = (n + pl.rowblocks - 1) / pl.rowblocks;
        pl.rowblocks = (n + pl.rows_per_block - 1) / pl.rows_per_block;
    }
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
#if CYTO_COLRED_PROBE
                CYTO_HIP(hipMemsetAsync(j.f_cnt, 0, nI + sizeof(int32_t), stream));     // (every row to the row builder)
#endif
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

    // ---- stage 2: the solver, one launch per phase for the whole batch ----
    std::vector<SolveJob> sj;
    for (F32Job &j : jobs) {
        if (j.alive() && j.h_nonfinite) j.status = CYTO_ERR_NONFINITE;
        if (j.alive())
            sj.push_back({j.dcost, j.dld, j.rowmap(), j.b_fws.as<float>(), j.b_iws.as<int32_t>(), j.b_ccol.as<uint32_t>(),
                          j.b_cval.as<float>(), j.b_misc.as<char>(), j.same(n), j.b_gid.as<int32_t>(), j.h_ngroups,
                          pl.wide ? &j.b_wide : j.b_chain});
    }
    DevBuf d_args[2];                                  // the chain solver's argument blocks: read by its kernels until the stream is drained
    const ChainPlan cp = {n, pl.cache, opts.chain_variant, opts.augmentation, opts.no_handover, opts.inject_exceptions,
                          opts.group_state_global, opts.aux_state_global, d_args};
    if (pl.wide) {
        const WidePlan wp = {n, opts.wide_rounds < 0 ? 0 : (opts.wide_rounds > 0 ? opts.wide_rounds : 4096 + (long long)n / 4),
                             opts.wide_rebuild, opts.wide_wipe, opts.wide_par, pl.cache};
        if (jobs[0].fused && !sj.empty()) {
            // few enough rows failed: the row builder takes those alone; otherwise (a few-cell-type matrix: the sampled minima lie too
            // far above the final ones) it builds every row as if there had been no lists
            F32Job &j = jobs[0];
            if (j.h_fused_failed <= n / 8) { sj[0].first_rows = j.f_rows; sj[0].first_count = j.h_fused_failed; }
            else j.h_fused_failed = n;
            g_fused_solves.fetch_add(1);
            g_fused_fallback_rows.fetch_add(j.h_fused_failed);
        }
        rc = wide_solve_batch(wp, sj, stream, e1c, e1d);
    } else
        rc = chain_solve_batch(cp, sj, stream, e1c, e1d);
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
        if (pl.wide) wide_note_status(h);
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
            if (pl.wide) wide_info(info, h); else chain_info(info, cp, h);
            info->row_groups = j.h_ngroups;
            info->certified = h_gap[0] >= 0.0 ? 1 : 0;
            info->gap_f64 = h_gap[0] >= 0.0 ? h_gap[0] : 0.0; info->gap_max_f64 = h_gap[0] >= 0.0 ? h_gap[1] : 0.0;
            info->gap_rows = h_gap[0] >= 0.0 ? (int64_t)h_gap[2] : 0;
            info->exact_status = ex.status; info->exact_edges = ex.edges; info->exact_free_rows = ex.free_rows;
            info->exact_changed_rows = ex.changed; info->exact_overflow_rows = ex.overflow;
            info->exact_ms_emit = ex.ms_emit; info->exact_ms_repair = ex.ms_repair;
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
