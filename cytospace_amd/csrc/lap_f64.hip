// lap_f64.hip -- the float64 LAP solver for gfx950 (MI355X): the precision of `lapjv(cost, force_doubles=True)` and of `lap.lapjv`, and
// the float64 polish of a float32 solve (cyto_lap_opts.polish; the exact option's way out when its edge set is over the cap).
//
// Kernel plan
//   colred_partial / colred_finish (lap_chain.h) / colred_assign (lap_jv.hip) : COLUMN REDUCTION, as in float32.
//   jv_chain<T, CH, COLSOL_LDS> : the generic dense chain (one 1024-thread workgroup, per-column state in registers), n <= 4 096.
//   build_row_caches_wide / jv_chain_stream : beyond that, per-column state in L2 and row caches for the row reduction.
//   widen_prices / widen_f32_rows : the warm start from a float32 solve's prices; the polish's float64 copy of the matrix.
// All of them are instantiated for double only.
//
// Compile with -ffp-contract=off (build.py does): the arithmetic is subtract/compare only,
// but nothing may be re-associated.
#include "cyto_common.h"
#include "lap_dev.h"
#include "lap_chain.h"
#include <math.h>
#include <vector>
#include <string.h>

namespace cyto {

// ------------------------------------------------------------------------------------------
// The sequential chain: REDUCTION TRANSFER -> AUGMENTING ROW REDUCTION x2 -> AUGMENTATION.
// ------------------------------------------------------------------------------------------
template <typename T> struct ChainArgs {
    int n;
    int64_t ld;
    const T *cost;
    T *v;                // [n] in: column minima; out: final prices
    T *u;                // [n] out
    int32_t *rowsol;     // [n] in/out
    int32_t *colsol;     // [n] in/out
    int32_t *matches;    // [n] in
    int32_t *freerows;   // [n] scratch
    int32_t *rtrows;     // [n] scratch
    int32_t *pred;       // [n] scratch
    double *total;       // [1] out
    long long *counters; // [C_NCOUNTERS] out
    int *status;         // [1] out (0 ok)
    T *dwork;            // [n] scratch (jv_chain_stream: distances)
    int32_t *lvl;        // [n] scratch (jv_chain_stream: level at which a column was scanned; 0 = not scanned)
    const uint32_t *cache_col;   // [n x 64] jv_chain_stream: row caches (build_row_caches_wide), or nullptr
    const T *cache_val;          // [n x 64]
    int cs_lds;                  // jv_chain_stream: colsol as u16 in LDS during RT / ARR (n <= 65 535)
    int v_lds;                   // jv_chain_stream: the prices in LDS too during RT / ARR (with cs_lds, where both fit)
};

template <typename T> __device__ __forceinline__ T ld_agent(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, int CH, bool COLSOL_LDS>
__global__ __launch_bounds__(BLOCK) void jv_chain(ChainArgs<T> a) {
    using V = typename VecOf<T>::type;
    constexpr int VW = VecOf<T>::W;
    constexpr int NC = CH * VW;
    static_assert(NC <= 64, "slot masks are 64-bit");
    extern __shared__ __attribute__((aligned(16))) int32_t s_colsol[];
    __shared__ RedScratch<T> red;

    const int tid = threadIdx.x;
    const int n = a.n;
    const int64_t ld = a.ld;
    const T *__restrict__ cost = a.cost;
    int par = 0;
    const T INF = (T)INFINITY;

    // slot s = m*VW + e  <->  column (m*BLOCK + tid)*VW + e
    auto slot_col = [&](int s) -> int { return ((s / VW) * BLOCK + tid) * VW + (s % VW); };
    uint64_t validm = 0;
#pragma unroll
    for (int s = 0; s < NC; s++) if (slot_col(s) < n) validm |= (1ull << s);

    auto colsol_get = [&](int j) -> int32_t { if constexpr (COLSOL_LDS) return s_colsol[j]; else return ld_i32(a.colsol + j); };
    auto colsol_set = [&](int j, int32_t i) { if constexpr (COLSOL_LDS) s_colsol[j] = i; else st_i32(a.colsol + j, i); };

    // ---- load prices and the assignment produced by the column reduction ----
    T vreg[NC];
    uint64_t assignedm = 0;
#pragma unroll
    for (int s = 0; s < NC; s++) {
        const int c = slot_col(s);
        vreg[s] = 0;
        if (c < n) {
            vreg[s] = a.v[c];
            const int32_t cs = a.colsol[c];
            if (cs >= 0) assignedm |= (1ull << s);
            if constexpr (COLSOL_LDS) s_colsol[c] = cs;
        }
    }

    auto load_row = [&](int i, V (&x)[CH]) {
        const V *rp = reinterpret_cast<const V *>(cost + (int64_t)i * ld);
#pragma unroll
        for (int m = 0; m < CH; m++) {
            const int q = m * BLOCK + tid;
            if (q * VW < n) x[m] = rp[q];
        }
    };
    // set vreg of column j (only its owner thread does anything)
    auto set_v = [&](int j, T val) {
        const int q = j / VW;
        if ((q % BLOCK) == tid) {
            const int s = (q / BLOCK) * VW + (j % VW);
#pragma unroll
            for (int t = 0; t < NC; t++) if (t == s) vreg[t] = val;
        }
    };
    auto set_assigned = [&](int j) {
        const int q = j / VW;
        if ((q % BLOCK) == tid) assignedm |= (1ull << ((q / BLOCK) * VW + (j % VW)));
    };

    long long c_rt = 0, c_arr = 0, c_auginit = 0, c_augrelax = 0, c_augs = 0, c_hops = 0;
    long long c_free_a1 = 0;

    // ---- free-row list (matches == 0) and reduction-transfer list (matches == 1), ascending ----
    int numfree = 0, nrt = 0;
    {
        const int R = (n + BLOCK - 1) / BLOCK;
        const int r0 = min(n, tid * R), r1 = min(n, r0 + R);
        int f = 0, g = 0;
        for (int i = r0; i < r1; i++) { const int mt = a.matches[i]; f += (mt == 0); g += (mt == 1); }
        int of = wg_exscan(f, red, par, &numfree);
        int og = wg_exscan(g, red, par, &nrt);
        for (int i = r0; i < r1; i++) {
            const int mt = a.matches[i];
            if (mt == 0) st_i32(a.freerows + of++, i);
            else if (mt == 1) st_i32(a.rtrows + og++, i);
        }
    }
    __syncthreads();
    const long long c_free_cr = numfree;

    // ---- REDUCTION TRANSFER ----
    if (n > 1) {
        for (int k = 0; k < nrt; k++) {
            const int i = ld_i32(a.rtrows + k);
            const int j1 = ld_i32(a.rowsol + i);
            V x[CH];
            load_row(i, x);
            Min1<T> loc; loc.u = INF; loc.k = 0xFFFFFFFFu; loc.a = 0;
#pragma unroll
            for (int s = 0; s < NC; s++) {
                const int c = slot_col(s);
                if (((validm >> s) & 1) && c != j1) {
                    const T h = vec_get<T>(x[s / VW], s % VW) - vreg[s];
                    if (h < loc.u) loc.u = h;
                }
            }
            loc.k = 0;  // value-only minimum
            const Min1<T> g = wg_min1(loc, red, par);
            // v[j1] = v[j1] - min  (owner only)
            {
                const int q = j1 / VW;
                if ((q % BLOCK) == tid) {
                    const int s = (q / BLOCK) * VW + (j1 % VW);
#pragma unroll
                    for (int t = 0; t < NC; t++) if (t == s) vreg[t] = vreg[t] - g.u;
                }
            }
            c_rt++;
        }
    }

    // ---- AUGMENTING ROW REDUCTION, two sweeps ----
    const long long arr_budget = 1000ll * n + 1000000ll;   // == JV_ARR_BUDGET(n) of the oracle
    for (int sweep = 0; sweep < 2; sweep++) {
        int k = 0;
        const int prev = numfree;
        numfree = 0;
        int carry = -1;
        while (carry >= 0 || k < prev) {
            if (c_arr >= arr_budget) {
                // step budget exhausted (see oracle/jv_oracle_impl.h): hand the waiting rows to the
                // augmentation phase, the displaced row first, then the rest in list order
                if (carry >= 0) { if (tid == 0) st_i32(a.freerows + numfree, carry); numfree++; carry = -1; }
                while (k < prev) { const int r = ld_i32(a.freerows + k); k++; if (tid == 0) st_i32(a.freerows + numfree, r); numfree++; }
                break;
            }
            int i;
            if (carry >= 0) { i = carry; carry = -1; }
            else { i = ld_i32(a.freerows + k); k++; }
            V x[CH];
            load_row(i, x);
            Top2<T> loc; loc.u1 = INF; loc.k1 = 0xFFFFFFFFu; loc.a1 = 0; loc.u2 = INF; loc.k2 = 0xFFFFFFFFu;
#pragma unroll
            for (int s = 0; s < NC; s++) {
                if ((validm >> s) & 1) {
                    const T h = vec_get<T>(x[s / VW], s % VW) - vreg[s];
                    top2_push(loc, h, (uint32_t)slot_col(s), vreg[s]);
                }
            }
            const Top2<T> g = wg_top2(loc, red, par);
            c_arr++;
            int j1 = (int)g.k1;
            const int j2 = (int)g.k2;
            int i0 = colsol_get(j1);
            const T vj1 = g.a1;
            const T vnew = vj1 - (g.u2 - g.u1);
            const bool lowers = vnew < vj1;
            if (lowers) set_v(j1, vnew);
            else if (i0 >= 0) { j1 = j2; i0 = colsol_get(j2); }
            __syncthreads();  // every wave has read colsol for this step before it changes
            if (tid == 0) { st_i32(a.rowsol + i, j1); colsol_set(j1, i); }
            set_assigned(j1);
            if (i0 >= 0) {
                if (lowers) carry = i0;
                else { if (tid == 0) st_i32(a.freerows + numfree, i0); numfree++; }
            }
        }
        __syncthreads();
        if (sweep == 0) c_free_a1 = numfree;
    }
    const long long c_free_a2 = numfree;

    // ---- AUGMENTATION ----
    int err = 0;
    for (int f = 0; f < numfree && !err; f++) {
        const int freerow = ld_i32(a.freerows + f);
        T dreg[NC];
        uint64_t scannedm = 0, readym = 0;
        {
            V x[CH];
            load_row(freerow, x);
#pragma unroll
            for (int s = 0; s < NC; s++) {
                dreg[s] = INF;
                if ((validm >> s) & 1) {
                    dreg[s] = vec_get<T>(x[s / VW], s % VW) - vreg[s];
                    a.pred[slot_col(s)] = freerow;
                }
            }
            c_auginit++;
        }
        bool have = false;
        T curmin = 0;
        int endofpath = -1;
        for (;;) {
            // pick: lexicographic min of (d, assigned?, column) over unscanned columns
            Min1<T> loc; loc.u = INF; loc.k = 0xFFFFFFFFu; loc.a = 0;
#pragma unroll
            for (int s = 0; s < NC; s++) {
                if (((validm & ~scannedm) >> s) & 1) {
                    const uint32_t key = (uint32_t)slot_col(s) | (((assignedm >> s) & 1) ? 0x80000000u : 0u);
                    if (lex_less(dreg[s], key, loc.u, loc.k)) { loc.u = dreg[s]; loc.k = key; loc.a = vreg[s]; }
                }
            }
            const Min1<T> g = wg_min1(loc, red, par);
            if (g.k == 0xFFFFFFFFu) { err = CYTO_ERR_INTERNAL; break; }
            const int jp = (int)(g.k & 0x7FFFFFFFu);
            if (!have || g.u != curmin) { readym |= scannedm; curmin = g.u; have = true; }
            if (!(g.k & 0x80000000u)) { endofpath = jp; break; }
            // scan column jp through its row
            {
                const int q = jp / VW;
                if ((q % BLOCK) == tid) scannedm |= (1ull << ((q / BLOCK) * VW + (jp % VW)));
            }
            const int i = colsol_get(jp);
            const T cip = cost[(int64_t)i * ld + jp];
            V x[CH];
            load_row(i, x);
            const T h = (cip - g.a) - curmin;
#pragma unroll
            for (int s = 0; s < NC; s++) {
                if (((validm & ~scannedm) >> s) & 1) {
                    const T v2 = (vec_get<T>(x[s / VW], s % VW) - vreg[s]) - h;
                    if (v2 < dreg[s]) { dreg[s] = v2; a.pred[slot_col(s)] = i; }
                }
            }
            c_augrelax++;
        }
        if (err) break;
        // price update: columns scanned at an earlier level than the final one
#pragma unroll
        for (int s = 0; s < NC; s++)
            if ((readym >> s) & 1) vreg[s] = (vreg[s] + dreg[s]) - curmin;
        set_assigned(endofpath);
        __syncthreads();  // pred stores of all waves are complete (and, via L2, visible)
        if (tid == 0) {
            int ep = endofpath, i;
            do {
                i = ld_i32(a.pred + ep);
                colsol_set(ep, i);
                const int j1 = ep;
                ep = ld_i32(a.rowsol + i);
                st_i32(a.rowsol + i, j1);
                c_hops++;
            } while (i != freerow);
        }
        c_augs++;
        __syncthreads();
    }

    // ---- write back prices and colsol, then duals u and the total ----
#pragma unroll
    for (int s = 0; s < NC; s++) {
        const int c = slot_col(s);
        if (c < n) {
            a.v[c] = vreg[s];
            if constexpr (COLSOL_LDS) a.colsol[c] = s_colsol[c];
        }
    }
    __threadfence_block();
    __syncthreads();
    double part = 0.0;
    for (int i = tid; i < n; i += BLOCK) {
        const int j = ld_i32(a.rowsol + i);
        const T cij = cost[(int64_t)i * ld + j];
        const T vj = __hip_atomic_load(a.v + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.u[i] = cij - vj;
        part += (double)cij;
    }
    // deterministic tree sum
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    __shared__ double s_sum[NW];
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < NW; w++) t += s_sum[w];
        *a.total = t;
        a.counters[C_RT] = c_rt; a.counters[C_ARR] = c_arr; a.counters[C_AUG_INIT] = c_auginit;
        a.counters[C_AUG_RELAX] = c_augrelax; a.counters[C_AUGS] = c_augs; a.counters[C_HOPS] = c_hops;
        a.counters[C_FREE_CR] = c_free_cr; a.counters[C_FREE_A1] = c_free_a1; a.counters[C_FREE_A2] = c_free_a2;
        a.counters[C_ROWS_READ] = c_rt + c_arr + c_auginit + c_augrelax;
        *a.status = err;
    }
}

// ------------------------------------------------------------------------------------------
// Row caches for jv_chain_stream (the float64 chain beyond n = 4 096): the idea of the float32 fast path (lap_jv.hip) -- prices
// only decrease during REDUCTION TRANSFER and AUGMENTING ROW REDUCTION, so the (at most) 63 columns of a row with the
// smallest reduced costs at build time, together with the 64th smallest reduced cost F (the floor), stay a certificate:
// a later scan whose second-smallest recomputed cached value is < F has found the row's exact lexicographic top-2 --
// in its simplest form.  One workgroup per row; the 64th smallest of the n order-preserving 64-bit keys is found bit by
// bit (64 counting passes over the row, which stays in L2), then the columns below it are written in column order with
// their raw costs.  Slot 63 holds the floor.
// ------------------------------------------------------------------------------------------
constexpr int WC_KC = 64;                          // slots per row; slot 63 = { sentinel, floor }
constexpr uint32_t WC_SENT = 0xFFFFFFFFu;
template <typename T> __device__ __forceinline__ uint64_t wide_ord(T h);
template <> __device__ __forceinline__ uint64_t wide_ord<double>(double h) {
    const uint64_t b = (uint64_t)__double_as_longlong(h + 0.0);
    return b ^ ((uint64_t)((int64_t)b >> 63) | 0x8000000000000000ull);
}
template <> __device__ __forceinline__ uint64_t wide_ord<float>(float h) {
    const uint32_t b = __float_as_uint(h + 0.0f);
    return (uint64_t)(b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u)) << 32;
}
template <typename T>
__global__ __launch_bounds__(256) void build_row_caches_wide(int n, int64_t ld, const T *__restrict__ cost, const T *__restrict__ v,
                                                             uint32_t *__restrict__ cache_col, T *__restrict__ cache_val) {
    __shared__ int s_cnt[2][4];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = blockIdx.x;
    const T *row = cost + (int64_t)i * ld;
    uint64_t K = 0;
    int par = 0;
    if (n >= WC_KC) {
        for (int b = 63; b >= 0; b--) {
            const uint64_t cand = K | (1ull << b);
            int c = 0;
            for (int j = tid; j < n; j += 256) c += wide_ord<T>(row[j] - v[j]) < cand;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0) s_cnt[par][w] = c;
            __syncthreads();
            const int tot = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
            par ^= 1;
            if (tot < WC_KC) K = cand;             // fewer than 64 keys below cand: the 64th smallest is >= cand
        }
    } else K = ~0ull;                              // fewer than 64 columns: all of them are cached, the floor is +inf
    // K is now the 64th smallest key: at most 63 keys are strictly below it, and its value is the floor
    if (tid == 0) { s_base = 0; if (n < WC_KC) cache_val[(int64_t)i * WC_KC + WC_KC - 1] = (T)INFINITY; }
    __syncthreads();
    for (int j0 = 0; j0 < n; j0 += 256) {
        const int j = j0 + tid;
        const T c = j < n ? row[j] : (T)0;
        const T h = j < n ? c - v[j] : (T)0;
        const uint64_t key = j < n ? wide_ord<T>(h) : ~0ull;
        const bool sel = j < n && key < K;
        if (j < n && n >= WC_KC && key == K) cache_val[(int64_t)i * WC_KC + WC_KC - 1] = h;   // (equal keys = equal values)
        const uint64_t m = __ballot(sel);
        if (lane == 0) s_cnt[par][w] = __builtin_popcountll(m);
        __syncthreads();
        int off = s_base;
        for (int ww = 0; ww < w; ww++) off += s_cnt[par][ww];
        const int tot = s_cnt[par][0] + s_cnt[par][1] + s_cnt[par][2] + s_cnt[par][3];
        if (sel) {
            const int pos = off + __builtin_popcountll(m & ((1ull << lane) - 1));
            cache_col[(int64_t)i * WC_KC + pos] = (uint32_t)j;
            cache_val[(int64_t)i * WC_KC + pos] = c;
        }
        __syncthreads();
        if (tid == 0) s_base = off + tot;          // (thread 0 is in wave 0: its off is the running base)
        par ^= 1;
        __syncthreads();
    }
    const int used = s_base;
    for (int p = used + tid; p < WC_KC; p += 256) {
        cache_col[(int64_t)i * WC_KC + p] = WC_SENT;
        if (p < WC_KC - 1) cache_val[(int64_t)i * WC_KC + p] = (T)0;
    }
}

// ------------------------------------------------------------------------------------------
// The same chain with every per-column quantity (prices, distances, predecessors, scan levels) in L2-resident
// global memory instead of VGPRs: jv_chain<double, CH> spills badly beyond CH = 2 (1024 threads leave 128 VGPRs
// per lane), this variant has no per-lane arrays at all and takes any n.  Column c is only ever touched by thread
// (c / VW) % BLOCK, so plain loads and stores in program order are all the ordering the per-column arrays need.
// A row scan = one coalesced sweep of the cost row (HBM) and of the price vector (L2).  Same arithmetic, same
// tie-breaking, same step budget as jv_chain / the oracle.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(BLOCK) void jv_chain_stream(ChainArgs<T> a) {
    using V = typename VecOf<T>::type;
    constexpr int VW = VecOf<T>::W;
    __shared__ RedScratch<T> red;
    __shared__ int s_run[4];
    __shared__ long long s_run_arr;
    // with the row caches (n <= 65 535): colsol lives in LDS as u16 during REDUCTION TRANSFER / AUGMENTING ROW REDUCTION -- the cached
    // step then gathers the owners from LDS and stores nothing but a lowered price to global memory (a load is only returned
    // after the stores issued before it are acknowledged)
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_cs[];
    // ... and, where they fit beside it (a.v_lds: n <= ~15 800 in float64), the prices too: the cached step then touches global
    // memory for the row's cache only
    const bool vl = a.v_lds != 0;
    T *const s_vT = reinterpret_cast<T *>(dyn_cs);
    uint16_t *const s_cs16 = reinterpret_cast<uint16_t *>(dyn_cs + (vl ? (((size_t)a.n * sizeof(T) + 15) & ~(size_t)15) : 0));
    const bool csl = a.cs_lds != 0;
#define V_GET(j) (vl ? s_vT[j] : ld_agent(v + (j)))
#define CS_GET(j) (csl ? (s_cs16[j] == 0xFFFFu ? -1 : (int32_t)s_cs16[j]) : ld_i32(a.colsol + (j)))
    const int tid = threadIdx.x;
    const int n = a.n;
    const int64_t ld = a.ld;
    const T *__restrict__ cost = a.cost;
    T *v = a.v, *d = a.dwork;
    int32_t *lvl = a.lvl, *pred = a.pred;
    int par = 0;
    const T INF = (T)INFINITY;
    const int nq = (n + VW - 1) / VW;                  // vector chunks per row (rows and v are VW-aligned and padded)
    const V *vp = reinterpret_cast<const V *>(v);

    long long c_rt = 0, c_arr = 0, c_auginit = 0, c_augrelax = 0, c_augs = 0, c_hops = 0, c_free_a1 = 0, c_dense = 0;
    const int lane = tid & 63;
    int numfree = 0, nrt = 0;
    {
        const int R = (n + BLOCK - 1) / BLOCK;
        const int r0 = min(n, tid * R), r1 = min(n, r0 + R);
        int f = 0, g = 0;
        for (int i = r0; i < r1; i++) { const int mt = a.matches[i]; f += (mt == 0); g += (mt == 1); }
        int of = wg_exscan(f, red, par, &numfree);
        int og = wg_exscan(g, red, par, &nrt);
        for (int i = r0; i < r1; i++) {
            const int mt = a.matches[i];
            if (mt == 0) st_i32(a.freerows + of++, i);
            else if (mt == 1) st_i32(a.rtrows + og++, i);
        }
    }
    if (csl) for (int c = tid; c < n; c += BLOCK) { const int32_t r = a.colsol[c]; s_cs16[c] = r < 0 ? (uint16_t)0xFFFFu : (uint16_t)r; }
    if (vl) for (int c = tid; c < n; c += BLOCK) s_vT[c] = v[c];
    __syncthreads();
    const long long c_free_cr = numfree;

    // ---- REDUCTION TRANSFER ----
    if (n > 1) {
        for (int k = 0; k < nrt; k++) {
            const int i = ld_i32(a.rtrows + k);
            const int j1 = ld_i32(a.rowsol + i);
            T mn = INF;
            bool certified = false;
            if (a.cache_col) {
                // cached scan, by every wave for itself (same loads, same result: no exchange needed)
                const uint32_t col = a.cache_col[(int64_t)i * WC_KC + lane];
                const T cv = a.cache_val[(int64_t)i * WC_KC + lane];
                const T F = __shfl(cv, WC_KC - 1);
                T h = INF;
                if (col != WC_SENT && (int)col != j1) h = cv - V_GET(col);
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) { const T o = __shfl_xor(h, off); h = o < h ? o : h; }
                mn = h;
                certified = mn < F;                    // every column outside the cache is still >= F
            }
            if (!certified) {
                const V *rp = reinterpret_cast<const V *>(cost + (int64_t)i * ld);
                Min1<T> loc; loc.u = INF; loc.k = 0; loc.a = 0;
                for (int q = tid; q < nq; q += BLOCK) {
                    const V x = rp[q], vv = vl ? reinterpret_cast<const V *>(s_vT)[q] : vp[q];
#pragma unroll
                    for (int e = 0; e < VW; e++) {
                        const int c = q * VW + e;
                        if (c < n && c != j1) { const T h = vec_get<T>(x, e) - vec_get<T>(vv, e); if (h < loc.u) loc.u = h; }
                    }
                }
                mn = wg_min1(loc, red, par).u;
                c_dense++;
            }
            if (((j1 / VW) % BLOCK) == tid) { if (vl) s_vT[j1] = s_vT[j1] - mn; else v[j1] = v[j1] - mn; }
            if (a.cache_col) __syncthreads();          // the new price has reached L2 (the barrier waits for the store) before any wave gathers it
            c_rt++;
        }
    }

    // ---- AUGMENTING ROW REDUCTION, two sweeps ----
    const long long arr_budget = 1000ll * n + 1000000ll;   // == JV_ARR_BUDGET(n) of the oracle
    for (int sweep = 0; sweep < 2; sweep++) {
        int k = 0;
        const int prev = numfree;
        numfree = 0;
        int carry = -1;
        while (carry >= 0 || k < prev) {
            int pend = -1;
            if (a.cache_col) {
                // ---- wave 0 alone follows the displacement chains while the row caches certify its scans: no barrier, no
                // other wave involved.  Lane = cache entry: the row's cache (requested as soon as the previous step knew the
                // next row), one round of gathers (price and owner of every cached column), the top-2 by wave shuffles,
                // the step's stores from lane 0 (agent scope: the wave's own later gathers see them, in L2).  It stops at the
                // first row whose cache does not certify its top-2 (that row is then scanned by the whole workgroup, below),
                // at the end of the sweep's list, or at the step budget. ----
                if (tid < 64) {
                    int pf_row = -1;
                    uint32_t pf_col = WC_SENT;
                    T pf_cv = 0;
                    while ((carry >= 0 || k < prev) && c_arr < arr_budget) {
                        const bool from_carry = carry >= 0;
                        const int i = from_carry ? carry : ld_i32(a.freerows + k);
                        uint32_t col; T cv;
                        if (pf_row == i) { col = pf_col; cv = pf_cv; }
                        else { col = ld_agent(a.cache_col + (int64_t)i * WC_KC + lane); cv = ld_agent(a.cache_val + (int64_t)i * WC_KC + lane); }
                        const T F = __shfl(cv, WC_KC - 1);
                        const bool valid = col != WC_SENT;
                        const T vj = V_GET(valid ? col : 0u);
                        const int32_t csj = CS_GET(valid ? col : 0u);
                        // the smallest reduced cost and its lane (cache rows are sorted by column: the lowest lane is the lowest
                        // column), then the smallest of the rest: reductions on order-preserving 64-bit keys, as in the float32 chain
                        const T h = valid ? cv - vj : INF;
                        const uint64_t kh = valid ? wide_ord<T>(h) : ~0ull;
                        const uint64_t m1 = wave_lexmin_u64(kh);
                        const int l1 = __builtin_ctzll(__ballot(kh == m1) | (1ull << 63));
                        int i0 = __shfl(csj, l1);
                        if (i0 >= 0 && m1 != ~0ull) {                         // (almost always) the next row of the chain: request its cache now
                            pf_row = i0;
                            pf_col = ld_agent(a.cache_col + (int64_t)i0 * WC_KC + lane);
                            pf_cv = ld_agent(a.cache_val + (int64_t)i0 * WC_KC + lane);
                        }
                        const uint64_t kh2 = lane == l1 ? ~0ull : kh;
                        const uint64_t m2 = wave_lexmin_u64(kh2);
                        const int l2 = __builtin_ctzll(__ballot(kh2 == m2) | (1ull << 63));
                        const T u1 = __shfl(h, l1), u2 = m2 == ~0ull ? INF : __shfl(h, l2);
                        if (from_carry) carry = -1; else k++;                 // the row is taken, certified or not
                        if (!(u2 < F)) { pend = i; break; }                   // (u2 < F: these are the row's exact lexicographic top-2)
                        c_arr++;
                        const int jfirst = (int)__shfl(col, l1);
                        int j1 = jfirst;
                        const int j2 = (int)__shfl(col, l2);
                        const T vj1 = __shfl(vj, l1);
                        const T vnew = vj1 - (u2 - u1);
                        const bool lowers = vnew < vj1;
                        if (!lowers && i0 >= 0) { j1 = j2; i0 = __shfl(csj, l2); }
                        if (lane == 0) {
                            if (lowers) { if (vl) s_vT[jfirst] = vnew; else __hip_atomic_store(v + jfirst, vnew, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
                            // (rowsol is not read during this phase and equals the inverse of colsol: rebuilt after it)
                            if (csl) s_cs16[j1] = (uint16_t)i; else st_i32(a.colsol + j1, i);
                            if (i0 >= 0 && !lowers) st_i32(a.freerows + numfree, i0);
                        }
                        if (i0 >= 0) { if (lowers) carry = i0; else numfree++; }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");       // the stores have reached L2
                    if (lane == 0) { s_run[0] = k; s_run[1] = carry; s_run[2] = numfree; s_run[3] = pend; s_run_arr = c_arr; }
                }
                __syncthreads();
                k = s_run[0]; carry = s_run[1]; numfree = s_run[2]; pend = s_run[3]; c_arr = s_run_arr;
                __syncthreads();                                             // (s_run is rewritten by the next run)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");           // wave 0's prices: drop what this CU's L1 holds
                if (pend < 0 && c_arr < arr_budget) continue;                // the sweep's list is exhausted
            }
            if (pend < 0 && c_arr >= arr_budget) {
                if (carry >= 0) { if (tid == 0) st_i32(a.freerows + numfree, carry); numfree++; carry = -1; }
                while (k < prev) { const int r = ld_i32(a.freerows + k); k++; if (tid == 0) st_i32(a.freerows + numfree, r); numfree++; }
                break;
            }
            int i;
            if (pend >= 0) i = pend;
            else if (carry >= 0) { i = carry; carry = -1; }
            else { i = ld_i32(a.freerows + k); k++; }
            Top2<T> g;
            const bool certified = false;
            if (!certified) {
                const V *rp = reinterpret_cast<const V *>(cost + (int64_t)i * ld);
                Top2<T> loc; loc.u1 = INF; loc.k1 = 0xFFFFFFFFu; loc.a1 = 0; loc.u2 = INF; loc.k2 = 0xFFFFFFFFu;
                for (int q = tid; q < nq; q += BLOCK) {
                    const V x = rp[q], vv = vl ? reinterpret_cast<const V *>(s_vT)[q] : vp[q];
#pragma unroll
                    for (int e = 0; e < VW; e++) {
                        const int c = q * VW + e;
                        if (c < n) top2_push(loc, vec_get<T>(x, e) - vec_get<T>(vv, e), (uint32_t)c, vec_get<T>(vv, e));
                    }
                }
                g = wg_top2(loc, red, par);
                c_dense++;
            }
            c_arr++;
            int j1 = (int)g.k1;
            const int j2 = (int)g.k2;
            int i0 = CS_GET(j1);
            const T vj1 = g.a1;
            const T vnew = vj1 - (g.u2 - g.u1);
            const bool lowers = vnew < vj1;
            if (lowers) { if (((j1 / VW) % BLOCK) == tid) { if (vl) s_vT[j1] = vnew; else v[j1] = vnew; } }
            else if (i0 >= 0) { j1 = j2; i0 = CS_GET(j2); }
            __syncthreads();  // every wave has read colsol for this step before it changes
            if (tid == 0) { if (csl) s_cs16[j1] = (uint16_t)i; else st_i32(a.colsol + j1, i); }
            if (i0 >= 0) {
                if (lowers) carry = i0;
                else { if (tid == 0) st_i32(a.freerows + numfree, i0); numfree++; }
            }
            __syncthreads();  // the colsol store is visible (L2) before the next step reads it
        }
        __syncthreads();
        if (sweep == 0) c_free_a1 = numfree;
    }
    const long long c_free_a2 = numfree;
    // colsol back to global memory, rowsol = its inverse (ARR kept only colsol current)
    __syncthreads();
    for (int c = tid; c < n; c += BLOCK) {
        const int32_t r = CS_GET(c);
        if (csl) a.colsol[c] = r;
        if (vl) v[c] = s_vT[c];
        if (r >= 0) a.rowsol[r] = c;
    }
    __threadfence();
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#undef CS_GET
#undef V_GET

    // ---- AUGMENTATION: relaxation and the search for the next pick share one sweep ----
    int err = 0;
    for (int f = 0; f < numfree && !err; f++) {
        const int freerow = ld_i32(a.freerows + f);
        Min1<T> loc; loc.u = INF; loc.k = 0xFFFFFFFFu; loc.a = 0;
        {
            const V *rp = reinterpret_cast<const V *>(cost + (int64_t)freerow * ld);
            for (int q = tid; q < nq; q += BLOCK) {
                const V x = rp[q], vv = vp[q];
#pragma unroll
                for (int e = 0; e < VW; e++) {
                    const int c = q * VW + e;
                    if (c < n) {
                        const T dd = vec_get<T>(x, e) - vec_get<T>(vv, e);
                        d[c] = dd; pred[c] = freerow; lvl[c] = 0;
                        const uint32_t key = (uint32_t)c | (ld_i32(a.colsol + c) >= 0 ? 0x80000000u : 0u);
                        if (lex_less(dd, key, loc.u, loc.k)) { loc.u = dd; loc.k = key; loc.a = vec_get<T>(vv, e); }
                    }
                }
            }
            c_auginit++;
        }
        bool have = false;
        T curmin = 0;
        int endofpath = -1, level = 0;
        for (;;) {
            const Min1<T> g = wg_min1(loc, red, par);
            if (g.k == 0xFFFFFFFFu) { err = CYTO_ERR_INTERNAL; break; }
            const int jp = (int)(g.k & 0x7FFFFFFFu);
            if (!have || g.u != curmin) { level++; curmin = g.u; have = true; }
            if (!(g.k & 0x80000000u)) { endofpath = jp; break; }
            if (((jp / VW) % BLOCK) == tid) lvl[jp] = level;                 // scanned (its d keeps the value at the pick)
            const int i = ld_i32(a.colsol + jp);
            const T cip = cost[(int64_t)i * ld + jp];
            const T h = (cip - g.a) - curmin;
            const V *rp = reinterpret_cast<const V *>(cost + (int64_t)i * ld);
            loc.u = INF; loc.k = 0xFFFFFFFFu; loc.a = 0;
            for (int q = tid; q < nq; q += BLOCK) {
                const V x = rp[q], vv = vp[q];
#pragma unroll
                for (int e = 0; e < VW; e++) {
                    const int c = q * VW + e;
                    if (c < n && lvl[c] == 0) {
                        const T v2 = (vec_get<T>(x, e) - vec_get<T>(vv, e)) - h;
                        T dc = d[c];
                        if (v2 < dc) { dc = v2; d[c] = v2; pred[c] = i; }
                        const uint32_t key = (uint32_t)c | (ld_i32(a.colsol + c) >= 0 ? 0x80000000u : 0u);
                        if (lex_less(dc, key, loc.u, loc.k)) { loc.u = dc; loc.k = key; loc.a = vec_get<T>(vv, e); }
                    }
                }
            }
            c_augrelax++;
        }
        if (err) break;
        // price update: columns scanned at an earlier level than the final one
        for (int q = tid; q < nq; q += BLOCK) {
#pragma unroll
            for (int e = 0; e < VW; e++) {
                const int c = q * VW + e;
                if (c < n) { const int lv = lvl[c]; if (lv != 0 && lv < level) v[c] = (v[c] + d[c]) - curmin; }
            }
        }
        __threadfence_block();
        __syncthreads();  // pred / price stores of all waves are complete (and, via L2, visible)
        if (tid == 0) {
            int ep = endofpath, i;
            do {
                i = ld_i32(pred + ep);
                st_i32(a.colsol + ep, i);
                const int j1 = ep;
                ep = ld_i32(a.rowsol + i);
                st_i32(a.rowsol + i, j1);
                c_hops++;
            } while (i != freerow);
        }
        c_augs++;
        __syncthreads();
    }

    // ---- duals u and the total ----
    __threadfence_block();
    __syncthreads();
    double part = 0.0;
    if (!err) {
        for (int i = tid; i < n; i += BLOCK) {
            const int j = ld_i32(a.rowsol + i);
            const T cij = cost[(int64_t)i * ld + j];
            const T vj = __hip_atomic_load(a.v + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.u[i] = cij - vj;
            part += (double)cij;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    __shared__ double s_sum[NW];
    if ((tid & 63) == 0) s_sum[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < NW; w++) t += s_sum[w];
        *a.total = t;
        a.counters[C_RT] = c_rt; a.counters[C_ARR] = c_arr; a.counters[C_AUG_INIT] = c_auginit;
        a.counters[C_AUG_RELAX] = c_augrelax; a.counters[C_AUGS] = c_augs; a.counters[C_HOPS] = c_hops;
        a.counters[C_FREE_CR] = c_free_cr; a.counters[C_FREE_A1] = c_free_a1; a.counters[C_FREE_A2] = c_free_a2;
        a.counters[C_ROWS_READ] = (a.cache_col ? c_dense : c_rt + c_arr) + c_auginit + c_augrelax;
        *a.status = err;
    }
}

// ---- float64 (the force_doubles / lapjv_compat precision): the generic chain, one problem ----
template <typename T, int CH, bool LDSCS>
static int launch_chain(const ChainArgs<T> &args, hipStream_t stream) {
    const size_t shmem = LDSCS ? (((size_t)args.n * sizeof(int32_t) + 15) / 16) * 16 : 16;
    auto kern = jv_chain<T, CH, LDSCS>;
    int rc = set_max_dynamic_lds(reinterpret_cast<const void *>(kern));
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(1), dim3(BLOCK), shmem, stream, args);
    CYTO_HIP(hipGetLastError());
    return CYTO_OK;
}

__global__ __launch_bounds__(256) void widen_prices(int n, const float *__restrict__ v32, double *__restrict__ v64) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) v64[j] = (double)v32[j];
}

// float64 (the precision of `lapjv(cost, force_doubles=True)` and of `lap.lapjv`, linear_assignment_solvers.py:13-15, 36).
// By default WARM-started (oracle/jv_oracle.c: jv_oracle_warm_f64): the classic float64 solve spends nearly all its time in the
// price wars of the row reduction, and the prices those wars converge to are known to float32 resolution beforehand -- the matrix is
// narrowed on the device, the float32 wide solver runs on it, its prices (widened exactly) are the start, every row free; the
// float64 augmenting row reduction then takes ~1.2 n steps instead of ~240 n and leaves a handful of rows to the augmentation.
// cyto_lap_opts.mode = 1 (or any chain option): the cold classic chain, the parity reference of rounds 1-3.
int lap_solve_f64(int n, const double *cost, int64_t ld, int cost_on_device, int32_t *rowsol, int32_t *colsol,
                  double *u, double *v, double *total, cyto_lap_info *info, int device_id, hipStream_t stream,
                  const cyto_lap_opts &opts, const float *warm_prices_host) {
    // warm_prices_host: the start prices are the caller's (the float32 solve of this very matrix: lap_polish_f64) -- no narrowing, no
    // float32 solve here
    typedef double T;
    constexpr int VW = VecOf<T>::W;
    if (n <= 0 || !cost || ld < n) return CYTO_ERR_BAD_ARG;
    int rc = check_opts(opts);
    if (rc) return rc;
    if (opts.exact) return CYTO_ERR_BAD_ARG;             // (the float32 solve's option: a float64 solve is exact already)
    if (n > FAST_NMAX) return CYTO_ERR_UNSUPPORTED;
    if ((rc = select_device(device_id))) return rc;
    Events<3> ev;
    if ((rc = ev.create())) return rc;
    const hipEvent_t e0 = ev[0], e1 = ev[1], e2 = ev[2];
    DevBuf staged;
    const T *dcost = cost;
    int64_t dld = ld;
    const bool aligned = cost_on_device && (ld % VW == 0) && ((reinterpret_cast<uintptr_t>(cost) & 15) == 0);
    if (!aligned) {
        dld = ((int64_t)n + VW - 1) / VW * VW;
        if ((rc = staged.alloc((size_t)n * dld * sizeof(T), stream))) return rc;
        CYTO_HIP(hipMemcpy2DAsync(staged.p, dld * sizeof(T), cost, ld * sizeof(T), (size_t)n * sizeof(T), n,
                                  cost_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        dcost = staged.as<T>();
    }
    const int colblocks = (n + 256 * VW - 1) / (256 * VW);
    int rowblocks = (2048 + colblocks - 1) / colblocks;
    rowblocks = max(1, min(rowblocks, (n + 15) / 16));
    const int rows_per_block = (n + rowblocks - 1) / rowblocks;
    rowblocks = (n + rows_per_block - 1) / rows_per_block;
    DevBuf b_fws, b_iws, b_imin, b_pmin, b_parg, b_misc;
    const size_t nT = (size_t)n * sizeof(T), nI = (size_t)n * sizeof(int32_t);
    if ((rc = b_fws.alloc(6 * nT + 64, stream)) || (rc = b_iws.alloc(10 * nI + 64, stream)) || (rc = b_imin.alloc(nI, stream)) ||
        (rc = b_pmin.alloc((size_t)rowblocks * nT, stream)) || (rc = b_parg.alloc((size_t)rowblocks * nI, stream)) ||
        (rc = b_misc.alloc(sizeof(LapStatus), stream)))
        return rc;
    T *d_v = b_fws.as<T>(), *d_u = b_fws.as<T>() + n;
    int32_t *d_rowsol = b_iws.as<int32_t>(), *d_colsol = d_rowsol + n, *d_matches = d_rowsol + 2 * (size_t)n;
    LapStatus *st = b_misc.as<LapStatus>();
    CYTO_HIP(hipMemsetAsync(st, 0, sizeof(LapStatus), stream));
    CYTO_HIP(hipMemsetAsync(d_rowsol, 0xFF, nI, stream));
    CYTO_HIP(hipMemsetAsync(d_matches, 0, nI, stream));
    CYTO_HIP(hipEventRecord(e0, stream));
    hipLaunchKernelGGL(colred_partial<T>, dim3(colblocks, rowblocks), dim3(256), 0, stream, n, dld, dcost, rows_per_block,
                       b_pmin.as<T>(), b_parg.as<int32_t>(), &st->nonfinite, n, (const int32_t *)nullptr, (const int32_t *)nullptr);
    int h_nonfinite = 0;
    CYTO_HIP(hipMemcpyAsync(&h_nonfinite, &st->nonfinite, sizeof(int), hipMemcpyDeviceToHost, stream));
    CYTO_HIP(hipStreamSynchronize(stream));
    if (h_nonfinite) return CYTO_ERR_NONFINITE;
    bool warm = opts.mode != 1 && opts.chain_variant == 0 && opts.augmentation == 0 && n >= 2;
    double ms_warm = 0.0;
    if (warm) {
        // the float32 wide solve of the narrowed matrix: its prices are the start
        const int64_t ld32 = ((int64_t)n + 3) & ~(int64_t)3;
        DevBuf d32, dv32;
        std::vector<float> h_v32((size_t)n);
        cyto_lap_info li32;
        if (warm_prices_host) {
            memset(&li32, 0, sizeof li32);
            memcpy(h_v32.data(), warm_prices_host, (size_t)n * sizeof(float));
            if ((rc = dv32.alloc((size_t)n * sizeof(float), stream))) return rc;
            rc = CYTO_OK;
        } else {
            if ((rc = d32.alloc((size_t)n * ld32 * sizeof(float), stream)) || (rc = dv32.alloc((size_t)n * sizeof(float), stream))) return rc;
            if ((rc = narrow_to_f32(n, dld, dcost, ld32, d32.as<float>(), stream))) return rc;
            rc = lap_solve_f32(n, d32.as<float>(), ld32, 1, nullptr, nullptr, nullptr, h_v32.data(), nullptr, &li32, device_id, stream, k_default_opts);
        }
        if (rc == CYTO_ERR_NONFINITE) { warm = false; rc = CYTO_OK; }       // finite float64 costs beyond float32's range: the cold start
        else if (rc) return rc;
        else {
            ms_warm = li32.ms_total;
            CYTO_HIP(hipMemcpyAsync(dv32.p, h_v32.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(widen_prices, dim3((n + 255) / 256), dim3(256), 0, stream, n, dv32.as<float>(), d_v);
            CYTO_HIP(hipMemsetAsync(d_colsol, 0xFF, nI, stream));     // nothing assigned, every row free (rowsol / matches: above)
            CYTO_HIP(hipGetLastError());
            CYTO_HIP(hipStreamSynchronize(stream));                    // (h_v32 / dv32 / d32 are locals)
        }
    }
    if (!warm) {
        hipLaunchKernelGGL(colred_finish<T>, dim3((n + 255) / 256), dim3(256), 0, stream, n, rowblocks, b_pmin.as<T>(),
                           b_parg.as<int32_t>(), d_v, b_imin.as<int32_t>(), d_rowsol, d_matches);
        launch_colred_assign(n, b_imin.as<int32_t>(), d_rowsol, d_colsol, stream);
    }
    CYTO_HIP(hipEventRecord(e1, stream));
    ChainArgs<T> ca;
    ca.n = n; ca.ld = dld; ca.cost = dcost; ca.v = d_v; ca.u = d_u;
    ca.rowsol = d_rowsol; ca.colsol = d_colsol; ca.matches = d_matches;
    ca.freerows = d_rowsol + 3 * (size_t)n; ca.rtrows = d_rowsol + 4 * (size_t)n; ca.pred = d_rowsol + 5 * (size_t)n;
    ca.total = &st->total; ca.counters = st->counters; ca.status = &st->status;
    ca.dwork = d_v + 4 * (size_t)n; ca.lvl = d_rowsol + 7 * (size_t)n;
    ca.cache_col = nullptr; ca.cache_val = nullptr; ca.cs_lds = 0; ca.v_lds = 0;
    // register-resident chain while it does not spill (n <= 4096), else everything streams from L2 -- with row caches
    // against the post-column-reduction prices for REDUCTION TRANSFER and AUGMENTING ROW REDUCTION
    // (opts.chain_variant == 2: without them, every scan reads its row)
    const int64_t per = (int64_t)VW * BLOCK;
    DevBuf b_ccol, b_cval;
    if (n <= 2 * per && opts.chain_variant == 0) rc = launch_chain<T, 2, true>(ca, stream);
    else {
        if (opts.chain_variant != 2) {
            if ((rc = b_ccol.alloc((size_t)n * WC_KC * sizeof(uint32_t), stream)) || (rc = b_cval.alloc((size_t)n * WC_KC * sizeof(T), stream))) return rc;
            hipLaunchKernelGGL(build_row_caches_wide<T>, dim3(n), dim3(256), 0, stream, n, dld, dcost, d_v, b_ccol.as<uint32_t>(), b_cval.as<T>());
            ca.cache_col = b_ccol.as<uint32_t>(); ca.cache_val = b_cval.as<T>();
        }
        // (chain_variant 3: the caches with colsol in global memory -- what n > 65 535 uses -- forced for the test-suite)
        ca.cs_lds = (ca.cache_col && n <= 65535 && opts.chain_variant != 3) ? 1 : 0;
        const size_t vbytes = (((size_t)n * sizeof(T)) + 15) & ~(size_t)15, csbytes = (((size_t)n * 2 + 15) / 16) * 16;
        ca.v_lds = (ca.cs_lds && vbytes + csbytes <= (size_t)LDS_DYNAMIC_MAX) ? 1 : 0;
        const size_t cs_lds = ca.cs_lds ? csbytes + (ca.v_lds ? vbytes : 0) : 16;
        if ((rc = set_max_dynamic_lds(reinterpret_cast<const void *>(jv_chain_stream<T>)))) return rc;
        hipLaunchKernelGGL(jv_chain_stream<T>, dim3(1), dim3(BLOCK), cs_lds, stream, ca);
        rc = hipGetLastError() == hipSuccess ? CYTO_OK : CYTO_ERR_HIP;
    }
    if (rc) return rc;
    CYTO_HIP(hipEventRecord(e2, stream));
    CYTO_HIP(hipStreamSynchronize(stream));
    LapStatus h;
    CYTO_HIP(hipMemcpy(&h, st, sizeof h, hipMemcpyDeviceToHost));
    if (rowsol) CYTO_HIP(hipMemcpy(rowsol, d_rowsol, nI, hipMemcpyDeviceToHost));
    if (colsol) CYTO_HIP(hipMemcpy(colsol, d_colsol, nI, hipMemcpyDeviceToHost));
    if (u) CYTO_HIP(hipMemcpy(u, d_u, nT, hipMemcpyDeviceToHost));
    if (v) CYTO_HIP(hipMemcpy(v, d_v, nT, hipMemcpyDeviceToHost));
    if (total) *total = h.total;
    if (info) {
        memset(info, 0, sizeof *info);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1); info->ms_colred = ms;      // (warm start: the float32 solve's launches and waits included)
        (void)hipEventElapsedTime(&ms, e1, e2); info->ms_chain = ms;
        info->ms_total = info->ms_colred + info->ms_chain;
        info->f64_warm = warm ? 1 : 0; info->f64_warm_ms = ms_warm;
        info_from_counters(info, n, h);
        info->hbm_row_reads = n + h.counters[C_ROWS_READ];
        info->aug_handover = -1;
        info->row_groups = n;
    }
    return h.status ? CYTO_ERR_INTERNAL : CYTO_OK;
}

// The float64 POLISH of a float32 solve (cyto_lap_opts.polish): the float32 solvers compare rounded reduced costs, so on a near-tie
// (two assignments whose totals differ by less than the rounding of the float32 duals, ~1e-8) which optimal-looking assignment comes
// out depends on their constants (DESIGN "Tried", round 5: phases ending at 128 rows instead of 64 left the few-cell-type 20 000^2
// instance 2e-8 above its optimum).  When the certificate (dual_gap_rows) cannot prove the result optimal, the matrix is widened to
// float64 on the device (exactly), the float32 prices are the start with every row free, and the float64 augmenting row reduction and
// augmentation of the force_doubles path run from there (any prices with nothing assigned are a valid JV state): ~1.2 n steps.  The
// result is the optimum of the float32 matrix in float64 arithmetic -- indices that depend on the MATRIX, not on the float32 solver.
// Costs n^2 x 8 bytes of device memory and several times the solve: an option, not the default.
__global__ __launch_bounds__(256) void widen_f32_rows(int n, int64_t lds_, const float *__restrict__ src, const int32_t *__restrict__ rowmap,
                                                      int64_t ldd, double *__restrict__ dst) {
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        const float *__restrict__ r = src + (int64_t)(rowmap ? rowmap[row] : row) * lds_;
        for (int c = blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) dst[row * ldd + c] = (double)r[c];
    }
}
int lap_polish_f64(int n, const float *cost, int64_t ld, int cost_on_device, const int32_t *rowmap_host, int nu, const float *v32,
                   int32_t *rowsol, int32_t *colsol, float *u, float *v, double *total, double *ms_out, int device_id,
                   hipStream_t stream) {
    int rc = select_device(device_id);
    if (rc) return rc;
    const int nstored = rowmap_host ? nu : n;
    const int64_t ldd = ((int64_t)n + 1) & ~(int64_t)1;
    DevBuf d64, staged, d_map;
    const float *dsrc = cost;
    int64_t dls = ld;
    if ((rc = d64.alloc((size_t)n * ldd * sizeof(double), stream))) return rc;
    if (!cost_on_device) {
        if ((rc = staged.alloc((size_t)nstored * n * sizeof(float), stream))) return rc;
        CYTO_HIP(hipMemcpy2DAsync(staged.p, (size_t)n * sizeof(float), cost, (size_t)ld * sizeof(float), (size_t)n * sizeof(float), nstored,
                                  hipMemcpyHostToDevice, stream));
        dsrc = staged.as<float>(); dls = n;
    }
    if (rowmap_host) {
        if ((rc = d_map.alloc((size_t)n * sizeof(int32_t), stream))) return rc;
        CYTO_HIP(hipMemcpyAsync(d_map.p, rowmap_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    hipLaunchKernelGGL(widen_f32_rows, matrix_copy_grid(n), dim3(256), 0, stream, n, dls, dsrc,
                       rowmap_host ? d_map.as<int32_t>() : (const int32_t *)nullptr, ldd, d64.as<double>());
    CYTO_HIP(hipGetLastError());
    CYTO_HIP(hipStreamSynchronize(stream));
    staged.reset();
    std::vector<double> u64((size_t)n), v64((size_t)n);
    cyto_lap_info li = {};
    rc = lap_solve_f64(n, d64.as<double>(), ldd, 1, rowsol, colsol, u64.data(), v64.data(), total, &li, device_id, stream, k_default_opts, v32);
    if (rc) return rc;
    if (u) for (int i = 0; i < n; i++) u[i] = (float)u64[(size_t)i];
    if (v) for (int i = 0; i < n; i++) v[i] = (float)v64[(size_t)i];
    if (ms_out) *ms_out = li.ms_total;
    return CYTO_OK;
}

}  // namespace cyto
